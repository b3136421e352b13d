"""The reduced density matrix on the GPU (csrc/lpp_rdm.hip, lpp_rdm_kernels.h) against the numpy block form of tests/rdm_reference.py.

The tolerance, wherever one is named: per block  K * 2^-52 * max_r rho[r, r]  with rho from numpy (rdm_reference.tolerance) -- K products and
K - 1 additions, each term bounded by sqrt(rho_rr rho_cc); derived, not measured."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import rdm_reference as ref
from helpers import chain
from lanczosplusplus_amd import LanczosEngine, LppError, geometry, rdm_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "lanczosplusplus_amd", "host", "lanczos")
GOLD = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu


def _ring(L):
    return chain(L, -1.0, True)


def _sector_size(L, nup, ndown, basis):
    return len(oracle.heis_basis(L, 1, nup)) if basis == "spin_half" else oracle.hubbard_basis_words(L, nup, ndown)[0].size


def _compare(got, want, exact=False):
    """block lists (the numpy side carries K): labels, alpha words, then the matrices, bit for bit or within the tolerance; returns the largest
    deviation in units of the tolerance"""
    assert [(g[0], g[1]) for g in got] == [(w[0], w[1]) for w in want]
    worst = 0.0
    for (ku, kd, ga, gm), (_, _, wa, wm, terms) in zip(got, want):
        assert np.array_equal(ga, wa) and gm.shape == wm.shape
        if exact:
            assert np.array_equal(gm, wm), (ku, kd)
        else:
            tol = ref.tolerance(wm, terms)
            dev = float(np.max(np.abs(gm - wm)))
            assert dev <= tol, (ku, kd, dev, tol)
            worst = max(worst, dev / tol) if tol > 0 else worst
    return worst


def _want_blocks(L, nup, ndown, split, psi, basis="hubbard"):
    """numpy blocks (k_up, k_down, alpha, rho, K)"""
    want = ref.blocks(L, nup, ndown, split, psi, basis)
    return [w + (b["terms"],) for w, b in zip(want, ref.plan(L, nup, ndown, split, basis)["blocks"])]


# ---- 1. exact integers: the lane maps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("L,nup,ndown,split,basis", [(8, 4, 4, 4, "hubbard"), (8, 4, 3, 3, "hubbard"), (10, 5, 5, 5, "hubbard"), (10, 5, 0, 5, "spin_half")])
def test_exact_integers(L, nup, ndown, split, basis, dtype):
    """psi with integer entries in [-3, 3]: every partial sum is exact in f64, so the result equals numpy's bit for bit whatever the order --
    any mistake in the operand or result lane maps, in the gather or in the row-index conjugate shows as a wrong integer"""
    n = _sector_size(L, nup, ndown, basis)
    rng = np.random.default_rng(1000 * L + 10 * split + nup)
    psi = rng.integers(-3, 4, n).astype(np.float64)
    if dtype == "c128":
        psi = psi + 1j * rng.integers(-3, 4, n)
    want = _want_blocks(L, nup, ndown, split, psi, basis)
    if dtype == "c128":
        assert any(np.max(np.abs(w[3].imag)) > 0 for w in want)
    with LanczosEngine(dtype=dtype) as e:
        got = e.reduced_density_matrix_of(psi, L, nup, ndown, split, basis)
    _compare(got, want, exact=True)


# ---- 2. random normalised vectors --------------------------------------------------------------------------------------------------------------
_PSI = {}


def _random_psi(L, nup, ndown, cplx):
    key = (L, nup, ndown, cplx)
    if key not in _PSI:
        psi = oracle.fill_random(_sector_size(L, nup, ndown, "hubbard"), 4321, cplx)
        _PSI[key] = psi / np.linalg.norm(psi)
        _PSI[key].setflags(write=False)
    return _PSI[key]


def _check_random(e, psi, L, nup, ndown, split):
    got = e.reduced_density_matrix_of(psi, L, nup, ndown, split)
    want = _want_blocks(L, nup, ndown, split, psi)
    worst = _compare(got, want)
    tr = sum(np.trace(m) for _, _, _, m in got)
    print("L=%d (%d,%d) split %d %s: %d blocks, largest deviation %.3f of the tolerance, trace - 1 = %.2e" % (L, nup, ndown, split, psi.dtype, len(got), worst, abs(tr - 1)))
    assert abs(tr - np.vdot(psi, psi)) <= 1e-13
    for _, _, _, m in got:
        assert np.array_equal(m, m.conj().T)  # Hermitian bit for bit
    again = e.reduced_density_matrix_of(psi, L, nup, ndown, split)
    for (_, _, _, m1), (_, _, _, m2) in zip(got, again):
        assert np.array_equal(m1.view(np.uint64), m2.view(np.uint64))  # fixed summation order


@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("split", [6, 1, 0])
def test_random_vector_L12(split, dtype):
    """L = 12 (6,6), 853,776 states.  split 6: d = 400, K = 400, several tiles both ways, K ranges of the smaller blocks; split 1: d = 1, K up to
    213,444: the split-K path; split 0: the norm."""
    L, nup, ndown = 12, 6, 6
    psi = _random_psi(L, nup, ndown, dtype == "c128")
    with LanczosEngine(dtype=dtype) as e:
        _check_random(e, psi, L, nup, ndown, split)


@pytest.mark.parametrize("dtype", ["f64", "c128"])
def test_results_that_cannot_fit_are_refused_before_any_launch(dtype):
    """L = 12 (6,6): split 12 is one block of d = N = 853,776 rows (5.8 TB as f64) and split 11 four blocks of d = C(11,5) C(11,5..6) = 213,444
    rows each (1.5 TB as f64): LPP_ERR_NOMEM with the sizes in the message.  (The issue lists split 11 among the cases to compare with numpy as
    'large d, K <= 4'; its result cannot exist on this part or in numpy, so the large-d-small-K case is compared for real in
    test_large_blocks_of_few_terms and split = L in test_split_at_the_last_site.)"""
    L, nup, ndown = 12, 6, 6
    psi = _random_psi(L, nup, ndown, dtype == "c128")
    with LanczosEngine(dtype=dtype) as e:
        for split in (12, 11):
            with pytest.raises(LppError) as ei:
                e.reduced_density_matrix_of(psi, L, nup, ndown, split)
            assert ei.value.status == 3 and "bytes" in str(ei.value)
        _check_random(e, psi, L, nup, ndown, 0)  # the engine is still usable


@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("L,nup,ndown,split", [(8, 4, 4, 7), (8, 4, 4, 6)])
def test_large_blocks_of_few_terms(L, nup, ndown, split, dtype):
    """large d, K <= 4: d up to 1225 with K = 1 (L = 8, split 7), d up to 400 with K <= 4 (split 6)"""
    psi = _random_psi(L, nup, ndown, dtype == "c128")
    assert max(b["terms"] for b in rdm_plan(L, nup, ndown, split)["blocks"]) <= 4
    with LanczosEngine(dtype=dtype) as e:
        _check_random(e, psi, L, nup, ndown, split)


@pytest.mark.parametrize("dtype", ["f64", "c128"])
def test_split_at_the_last_site(dtype):
    """split = L on L = 6 (3,3): one block, d = N = 400, K = 1 -- the outer product conj(psi) psi^T"""
    L, nup, ndown = 6, 3, 3
    psi = _random_psi(L, nup, ndown, dtype == "c128")
    with LanczosEngine(dtype=dtype) as e:
        _check_random(e, psi, L, nup, ndown, L)
        (_, _, _, m), = e.reduced_density_matrix_of(psi, L, nup, ndown, L)
        # one product per element, rounded here and in numpy: each side is within 2^-52 |psi|_max^2 of the exact product (complex: two products and a sum)
        assert np.max(np.abs(m - np.outer(psi.conj(), psi))) <= 4 * 2.0 ** -52 * np.max(np.abs(psi)) ** 2


# ---- 3. closed form ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split,entropy", [(3, 1.46798265909749), (4, 1.13949696884325)])
def test_slater_product_state_has_the_free_fermion_entropy(split, entropy):
    """the Slater product state of the open 8-site chain, 4 up 4 down (amplitudes = minors of the hopping matrix's eigenvectors), needs no
    Lanczos: its entanglement entropy is 2 sum -[nu ln nu + (1 - nu) ln(1 - nu)], nu the eigenvalues of the split x split corner of <c+_i c_j>"""
    L, n = 8, 4
    _, phi = np.linalg.eigh(chain(L, -1.0))
    phi = phi[:, :n]
    words = oracle.onespin_basis(L, n)
    one = np.array([np.linalg.det(phi[[i for i in range(L) if (int(w) >> i) & 1], :]) for w in words])
    psi = np.kron(one, one)  # index = i_up + i_down * N_up
    nu = np.linalg.eigvalsh((phi @ phi.T)[:split, :split])
    nu = nu[(nu > 1e-15) & (nu < 1 - 1e-15)]
    want = 2 * float(np.sum(-(nu * np.log(nu) + (1 - nu) * np.log(1 - nu))))
    assert abs(want - entropy) <= 1e-12
    with LanczosEngine() as e:
        lam = np.concatenate([np.linalg.eigvalsh(m) for _, _, _, m in e.reduced_density_matrix_of(psi, L, n, n, split)])
    lam = lam[lam > 0]
    got = float(-np.sum(lam * np.log(lam)))
    print("split %d: entropy %.14f, free fermions %.14f" % (split, got, want))
    assert abs(got - want) <= 1e-11


# ---- 4. through the engine -----------------------------------------------------------------------------------------------------------------------
# the environment dictionaries and predicates of LAYOUTS in tests/test_gpu_observables.py (copied: that file's dictionary is never touched)
LAYOUTS = {
    "general": (dict(LPP_PRODUCT_LAYOUT="0"), lambda lay: lay["kernel"] != 4),
    "product_chained": (dict(LPP_PRODUCT_LAYOUT="1", LPP_PB_PERM="0"), lambda lay: lay["kernel"] == 4 and lay["chained_step"] == 1 and lay["rows_by_list_length"] == 0),
    "list_length_order": (dict(LPP_PRODUCT_LAYOUT="1"), lambda lay: lay["kernel"] == 4 and lay["rows_by_list_length"] == 1),
    "segmented": (dict(LPP_PRODUCT_LAYOUT="1", LPP_PB_PIECE_ROWS="256", LPP_PB_SEG="1"), lambda lay: lay["kernel"] == 4 and lay["segments"] == 4),
}
_BY_LAYOUT = {}
# (12, 6, 5) is the sector at which tests/test_gpu_observables.py holds these predicates.  At the issue's L = 8 (4,4) they cannot hold -- N_up = 70
# is below the 128 rows from which rows are stored by list length, and one LDS window holds the whole row block, so nothing is chained or
# segmented -- so L = 8 runs under the same four environments with the layout the engine then picks, and the predicates are asserted at L = 12.
SECTORS = {"L8": (8, 4, 4, False), "L12": (12, 6, 5, True)}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("sector", list(SECTORS))
def test_ground_state_of_the_hubbard_ring(sector, layout, monkeypatch):
    """ring, U = 4, split 4 of the resident ground state under every layout's environment: equal to the numpy blocks of e.state(0) within the
    tolerance, and the same matrix across the layouts to 1e-12 (the states differ by the solves' rounding, not the kernel's)"""
    env, check_layout = LAYOUTS[layout]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L, nup, ndown, predicate = SECTORS[sector]
    with LanczosEngine() as e:
        e.assemble_hubbard(L, nup, ndown, _ring(L), np.full(L, 4.0))
        lay = e.layout()
        assert not predicate or check_layout(lay), lay
        e.keep_states(1)
        e.lanczos(1, want_vectors=False)
        got = e.reduced_density_matrix(split=4)
        worst = _compare(got, _want_blocks(L, nup, ndown, 4, e.state(0)))
        w, labels = e.entanglement_spectrum(4)
        assert len(w) == 4 ** 4 == len(labels) and np.all(np.diff(w) >= 0)
        assert abs(np.sum(w) - 1) <= 1e-12 and w[0] >= -1e-14
        s = e.entanglement_entropy(4)
        assert abs(s + np.sum(w[w > 0] * np.log(w[w > 0]))) <= 1e-13 and 0.5 < s < 4 * np.log(4)
    first = _BY_LAYOUT.setdefault(sector, got)
    across = max(np.max(np.abs(m0 - m1)) for (_, _, _, m0), (_, _, _, m1) in zip(first, got))
    print("%s %s: kernel %d chained %d by list length %d segments %d; %.3f of the tolerance; across layouts %.3e; entropy %.12f"
          % (sector, layout, lay["kernel"], lay["chained_step"], lay["rows_by_list_length"], lay["segments"], worst, across, s))
    assert across <= 1e-12


def test_ground_state_of_the_heisenberg_ring():
    L, m = 10, 5
    with LanczosEngine() as e:
        e.assemble_heisenberg(L, m, chain(L, 1.0, True), chain(L, 1.0, True))
        e.keep_states(1)
        e.lanczos(1, want_vectors=False)
        got = e.reduced_density_matrix(split=4)
        _compare(got, _want_blocks(L, m, 0, 4, e.state(0), "spin_half"))
        w, _ = e.entanglement_spectrum(4)
        assert len(w) == 2 ** 4 and abs(np.sum(w) - 1) <= 1e-12 and w[0] >= -1e-14


@pytest.mark.parametrize("how", ["assemble_hubbard", "setup_hubbard_onthefly"])
def test_dense_matrix_equals_the_literal_loop(how):
    """dense=True is the reference's 4^split square matrix, rows by alpha: L = 6 (3,3) split 2 against the double loop"""
    L, nup, ndown, split = 6, 3, 3, 2
    with LanczosEngine() as e:
        getattr(e, how)(L, nup, ndown, _ring(L), np.full(L, 4.0))
        e.keep_states(1)
        e.lanczos(1, want_vectors=False)
        got = e.reduced_density_matrix(split, dense=True)
        want = ref.literal(L, nup, ndown, split, e.state(0))
        assert got.shape == (16, 16)
        assert np.max(np.abs(got - want)) <= 400 * 2.0 ** -52 * np.max(np.abs(np.diag(want)))
        with pytest.raises(ValueError):
            e.reduced_density_matrix_of(np.zeros(1), 8, 4, 4, 7, dense=True)  # 4^7 rows


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    with LanczosEngine() as e:
        e.assemble_hubbard(8, 4, 4, _ring(8), np.full(8, 4.0))
        with pytest.raises(LppError) as ei:
            e.reduced_density_matrix(4)  # nothing kept
        assert ei.value.status == 5
        with pytest.raises(ValueError):
            e.reduced_density_matrix_of(np.zeros(4899), 8, 4, 4, 4)
        with pytest.raises(LppError) as ei:
            e.reduced_density_matrix_of(np.zeros(4900), 8, 4, 4, 9)
        assert ei.value.status == 1
        e.keep_states(1)
        e.lanczos(1, want_vectors=False)
        import ctypes as C
        st = e._lib.lpp_engine_state_reduced_density_matrix(e._h, 0, 0, 8, 4, 3, 4, C.c_void_p())  # not the sector of the resident state
        assert st == 1
        assert e._lib.lpp_engine_state_reduced_density_matrix(e._h, 1, 0, 8, 4, 4, 4, C.c_void_p()) == 5  # one state kept
    with LanczosEngine() as e:
        with pytest.raises(LppError) as ei:
            e.reduced_density_matrix(2)  # no model
        assert ei.value.status == 5
        e.assemble_heisenberg(6, 6, chain(6, 1.0, True), chain(6, 1.0, True), twiceS=2)
        e.keep_states(1)
        with pytest.raises((LppError, ValueError)) as ei:
            e.reduced_density_matrix(2)
        assert "twiceS" in str(ei.value)
    L = 12
    monkeypatch.setenv("LPP_TJ_LAYOUT", "1")  # as test_new_entry_points_refuse_tj_engines sets one up
    with LanczosEngine() as e:
        hop = _ring(L)
        e.assemble_tj(L, 4, 4, hop, 0.5 * np.abs(hop), 0.5 * np.abs(hop), np.zeros((L, L)))
        assert e.layout()["kernel"] == 5
        with pytest.raises(LppError) as ei:
            e.reduced_density_matrix_of(np.zeros(4900), 8, 4, 4, 4)
        assert ei.value.status == 5
        with pytest.raises(LppError) as ei:
            e.bench_rdm(8, 4, 4, 4)
        assert ei.value.status == 5
        with pytest.raises(LppError) as ei:
            e.reduced_density_matrix(4)
        assert ei.value.status == 5


# ---- 6. the driver ---------------------------------------------------------------------------------------------------------------------------------
def test_driver_reduced_density_matrix():
    """lanczos -f tests/golden/hubbard_ladder_2x4.inp -r 4 -p 12: the three headings, the merged eigenvalues against entanglement_spectrum of the
    Python path on the same input (1e-9: the bar the driver tests hold printed values to), and the EntanglementEntropy= line"""
    assert os.path.exists(DRIVER), "run __graft_entry__.build()"
    path = os.path.join(GOLD, "hubbard_ladder_2x4.inp")
    res = subprocess.run([DRIVER, "-f", path, "-r", "4", "-p", "12"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    for heading in ("Reduced Density Matrix", "Eigenvectors of Reduced Density Matrix", "Eigenvalues of Reduced Density Matrix"):
        assert heading in lines, heading
    assert any(re.match(r"^# block k_up=\d+ k_down=\d+ dim=\d+$", ln) for ln in lines)
    k = lines.index("Eigenvalues of Reduced Density Matrix")
    count = int(lines[k + 1])
    got = np.array([float(x) for x in " ".join(lines[k + 2:]).split("EntanglementEntropy=")[0].split()])
    assert len(got) == count
    entropy = float(next(ln for ln in lines if ln.startswith("EntanglementEntropy=")).split("=")[1])
    inp = geometry.parse_input(open(path).read())
    L, nup, ndown = int(inp["TotalNumberOfSites"]), int(inp["TargetElectronsUp"]), int(inp["TargetElectronsDown"])
    with LanczosEngine() as e:
        e.assemble_hubbard(L, nup, ndown, geometry.terms_from_input(inp)[0], inp["hubbardU"], inp["potentialV"])
        e.keep_states(1)
        e.lanczos(1, init=oracle.fill_random(e.rows(), 1234), want_vectors=False)
        want, _ = e.entanglement_spectrum(4)
        s = e.entanglement_entropy(4)
    assert len(want) == count
    print("driver -r 4: %d eigenvalues, max deviation %.3e, entropy %.12g against %.12g" % (count, np.max(np.abs(got - want)), entropy, s))
    assert np.max(np.abs(got - want)) <= 1e-9 and np.all(np.diff(got) >= 0)
    assert abs(entropy - s) <= 1e-9
