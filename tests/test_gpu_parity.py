"""-m gpu: parity of the HIP path (through the C ABI) against the CPU oracle on the same inputs.

Tolerances: indices/structure bit-exact; matrix values bit-exact; SpMV 1e-13 relative per vector
(summation order differs); energies 1e-10 relative (BASELINE.json north_star).
"""
import os
from math import comb

import numpy as np
import pytest
import torch  # noqa: F401  (ThreadComm's buffers: loaded before the engine library, so that both use one HIP runtime -- INTEGRATION.md)

import oracle
from helpers import chain, rel, square
from lanczosplusplus_amd import LanczosEngine, LppError, tridiag_lowest

pytestmark = pytest.mark.gpu

E_TOL = 1e-10
SPMV_TOL = 1e-13


def models():
    L = 8
    out = {}
    out["hubbard"] = oracle.hubbard_csr(L, 4, 4, chain(L, -1.0), np.full(L, 4.0), np.linspace(-0.3, 0.3, 2 * L))
    out["heisenberg"] = oracle.heis_csr(12, 1, 6, chain(12, 1.0, True), chain(12, 1.0, True))
    hop = chain(L, -1.0).astype(complex)
    hop[0, 1] = -1.0 * np.exp(0.3j)
    hop[1, 0] = np.conj(hop[0, 1])
    out["tj_complex"] = oracle.tj_csr(L, 3, 3, chain(L, -1.0), chain(L, 0.4), chain(L, 0.4), chain(L, -0.1),
                                      force_complex=True)
    out["hubbard_complex"] = oracle.hubbard_csr(6, 3, 3, hop[:6, :6], np.full(6, 2.0))
    return out


@pytest.fixture(scope="module")
def mats():
    return models()


@pytest.mark.parametrize("name", ["hubbard", "heisenberg", "tj_complex", "hubbard_complex"])
@pytest.mark.parametrize("kernel", [0, 1, 2, 3])
@pytest.mark.parametrize("compress", [0, -1])
def test_spmv_acc_matches_oracle(mats, name, kernel, compress):
    A = mats[name]
    dt = "c128" if A.is_complex else "f64"
    with LanczosEngine(dtype=dt, spmv_kernel=kernel, compress_values=compress) as e:
        e.set_csr(A.rowptr, A.colind, A.values)
        assert e.rows() == A.nrows
        x0 = oracle.fill_random(A.nrows, 7, A.is_complex)
        y = oracle.fill_random(A.nrows, 8, A.is_complex)
        xg = e.matrixVectorProduct(x0.copy(), y)
        xo = oracle.spmv_acc(A, x0.copy(), y)
        assert rel(xg, xo) < SPMV_TOL
        # accumulate semantics: a second call adds H y again
        xg2 = e.matrixVectorProduct(xg.copy(), y)
        assert rel(xg2 - xg, xo - x0) < 1e-12


def test_value_dictionary_is_lossless_and_falls_back():
    """<= 256 distinct doubles: values are stored as 8-bit codes and decode bit-exactly; otherwise plain storage."""
    rng = np.random.default_rng(3)
    n = 3000
    import scipy.sparse as sp
    M = sp.random(n, n, density=0.004, random_state=7, format="csr")
    for distinct in (7, 5000):
        pool = rng.normal(size=distinct)
        M.data = pool[rng.integers(0, distinct, size=M.nnz)]
        rp, ci, va = M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data.copy()
        y = rng.normal(size=n)
        ref = M @ y
        for kernel in (2, 3):
            with LanczosEngine(spmv_kernel=kernel, compress_values=-1) as e:
                e.set_csr(rp, ci, va)
                g = e.get_csr()
                assert np.array_equal(g[0], rp) and np.array_equal(g[1], ci)
                assert np.array_equal(g[2].view(np.uint64), va.view(np.uint64))
                x = e.matrixVectorProduct(np.zeros(n), y)
                assert rel(x, ref) < 1e-13


def test_spmv_edge_cases():
    # empty rows, a single dense row, 1x1 matrix
    rowptr = np.array([0, 0, 3, 3, 4], np.int64)
    col = np.array([0, 1, 3, 2], np.int32)
    val = np.array([1.0, 2.0, 3.0, -1.0])
    with LanczosEngine() as e:
        e.set_csr(rowptr, col, val)
        x = np.ones(4)
        y = np.array([1.0, 10.0, 100.0, 1000.0])
        e.matrixVectorProduct(x, y)
        assert np.array_equal(x, np.array([1.0, 1 + 1 + 20 + 3000, 1.0, 1 - 100.0]))
        e.set_csr(np.array([0, 1], np.int64), np.array([0], np.int32), np.array([2.5]))
        x = np.array([1.0])
        e.matrixVectorProduct(x, np.array([2.0]))
        assert x[0] == 6.0
        eigs, zs, st = e.lanczos(1)
        assert abs(eigs[0] - 2.5) < 1e-14
    n = 300
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = n  # row 0 dense, others empty
    col = np.arange(n, dtype=np.int32)
    val = np.arange(1, n + 1, dtype=np.float64)
    with LanczosEngine(spmv_kernel=2) as e:
        e.set_csr(rowptr, col, val)
        x = np.zeros(n)
        e.matrixVectorProduct(x, np.ones(n))
        assert x[0] == n * (n + 1) / 2 and not x[1:].any()


def test_errors_are_loud():
    with LanczosEngine() as e:
        with pytest.raises(LppError):
            e.lanczos(1)  # no matrix
        with pytest.raises(LppError):
            e.set_csr(np.array([0, 1], np.int64), np.array([5], np.int32), np.array([1.0]))  # column out of range


def test_model_setup_rejections_keep_their_status_and_text():
    """What the model set-up entry points refuse, and with which words: the C entry points themselves (the ctypes library on e._h, so the
    Python wrappers' own checks cannot answer first).  Single GPU: every refusal comes before any change of state -- the installed matrix
    gives the same product, bit for bit, after each.  Two ranks: the checks of the partition and of the transposition-exchange geometry,
    on rank 0 of a two-rank thread group with no second thread (every row returns before a collective); status and text only."""
    import ctypes as C

    from lanczosplusplus_amd import _capi
    from lanczosplusplus_amd.comm import ThreadComm, ThreadGroup
    lib = _capi.lib()
    INVALID = _capi.LPP_ERR_INVALID
    L, n = 8, 4
    N = comb(L, n)  # 70 states per species
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    hop, zero = chain(L, -1.0), np.zeros((L, L))
    him = np.zeros((L, L))
    him[0, 1], him[1, 0] = 0.3, -0.3
    jc = chain(L, 0.5)
    U, V, pot = np.full(L, 4.0), np.zeros(L), np.zeros(2 * L)

    def refused(status, text, at_start=False):
        msg = lib.lpp_last_error().decode()
        print(status, msg)
        assert status == INVALID, (status, msg)
        assert msg.startswith(text) if at_start else text in msg, msg

    with LanczosEngine() as e:
        h = e._h
        e.assemble_hubbard(L, n, n, hop, U)
        y = oracle.fill_random(N * N, 8)
        want = e.matrixVectorProduct(np.zeros(N * N), y).tobytes()
        rows = [
            (lambda: lib.lpp_engine_assemble_hubbard_super(h, None, 32, n, n, vp(hop), None, vp(U), vp(V), None, None),
             "lpp_engine_assemble_hubbard: bad argument"),
            (lambda: lib.lpp_engine_assemble_hubbard_super(h, None, L, n, n, vp(hop), vp(him), vp(U), vp(V), None, None),
             "complex couplings need a c128 engine"),
            (lambda: lib.lpp_engine_setup_hubbard_onthefly_ext(h, None, L, n, n, vp(hop), vp(him), vp(U), vp(V), None),
             "setup_hubbard_onthefly: complex hoppings need a c128 engine"),
            (lambda: lib.lpp_engine_assemble_tj(h, L, 5, 4, vp(hop), None, vp(jc), vp(jc), vp(zero), None, 0),
             "lpp_engine_assemble_tj: bad argument"),
            (lambda: lib.lpp_engine_assemble_tj(h, L, 3, 3, vp(hop), None, vp(jc), vp(jc), vp(zero), vp(pot), L),
             "potentialV needs 2*L entries"),
            (lambda: lib.lpp_engine_assemble_heisenberg(h, L, L + 1, vp(jc), vp(jc), None, 0),
             "lpp_engine_assemble_heisenberg: bad argument"),
            (lambda: lib.lpp_engine_set_model_tj(h, L, 5, 4, vp(hop), None, vp(jc), vp(jc), vp(zero), None, 0),
             "lpp_engine_set_model_tj: bad argument"),
        ]
        for call, text in rows:
            refused(call(), text)
            assert e.matrixVectorProduct(np.zeros(N * N), y).tobytes() == want, text

    per = -(-N // 2)  # 35 down configurations per rank
    chunk = lib.lpp_xchg_chunk(N, N, 2)
    assert (per, chunk) == (35, 1680)
    comm = ThreadComm(ThreadGroup(2, torch.device("cuda", 0)), 0, per * N, 200, False, xchg_chunk=chunk)

    def with_(**changed):  # the communicator with some fields set differently
        s = _capi.Comm()
        for name, _ in _capi.Comm._fields_:
            setattr(s, name, changed.get(name, getattr(comm.struct, name)))
        return C.byref(s)

    short = per * 16  # 16 up indices per rank: 32 < 70 in all
    with comm.stream_context(), LanczosEngine(max_steps=200, stream=comm.stream_handle) as e:
        h = e._h
        refused(lib.lpp_engine_setup_hubbard_onthefly_super(h, with_(), L, n, n, vp(hop), None, vp(U), vp(V), None, vp(jc)), "runs on one GPU")
        refused(lib.lpp_engine_assemble_hubbard_super(h, with_(shard_stride=per * N + 1), L, n, n, vp(hop), None, vp(U), vp(V), None, None),
                "shard_stride must be ceil(N_down/nranks)*N_up")
        refused(lib.lpp_engine_assemble_hubbard_super(h, with_(), L, n, n, vp(hop), None, vp(U), vp(V), None, vp(jc)), "need the all-gather exchange")
        refused(lib.lpp_engine_assemble_hubbard_super(h, with_(xchg_chunk=short), L, n, n, vp(hop), None, vp(U), vp(V), None, None),
                "assemble_hubbard: transposition exchange needs send2/recv2")
        # the one-species matrix of this sector takes the packed layout, so of the two sentences this entry point has for the
        # transposition exchange it is the geometry's that answers ("setup_hubbard_onthefly: transposition exchange needs ...")
        refused(lib.lpp_engine_setup_hubbard_onthefly_ext(h, with_(xchg_chunk=short), L, n, n, vp(hop), None, vp(U), vp(V), None),
                "setup_hubbard_onthefly:", at_start=True)


@pytest.mark.parametrize("name", ["hubbard", "heisenberg", "tj_complex", "hubbard_complex"])
@pytest.mark.parametrize("kernel", [0, 1, 2, 3])
def test_lanczos_energy_and_coefficients(mats, name, kernel):
    A = mats[name]
    dt = "c128" if A.is_complex else "f64"
    init = oracle.fill_random(A.nrows, 1234, A.is_complex)
    eo, zo, so = oracle.lanczos_solve(A, init, nstates=1)
    steps_o, ao, bo, _, _ = oracle.lanczos_decomposition(A, init)
    with LanczosEngine(dtype=dt, spmv_kernel=kernel) as e:
        e.set_csr(A.rowptr, A.colind, A.values)
        # built-in start vector (init=None) is the same splitmix64 stream as the oracle's
        eg, zg, st = e.lanczos(1, want_vectors=True)
        assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0])
        assert st["steps"] == so
        r = oracle.spmv_acc(A, np.zeros_like(zg[0]), zg[0]) - eg[0] * zg[0]
        assert np.linalg.norm(r) < 1e-5
        assert abs(np.linalg.norm(zg[0]) - 1) < 1e-8
        ag, bg, st2 = e.decomposition(init)
        assert len(ag) == steps_o
        assert rel(ag, ao) < 1e-8 and rel(bg, bo) < 1e-8
        # dense cross-check
        ed = np.linalg.eigvalsh(A.to_scipy().toarray())[0]
        assert abs(eg[0] - ed) <= 1e-10 * abs(ed)


@pytest.mark.parametrize("save", [0, 1])
def test_ritz_vectors_two_pass_equals_saved(mats, save):
    A = mats["hubbard"]
    with LanczosEngine(save_vectors=save) as e:
        e.set_csr(A.rowptr, A.colind, A.values)
        eg, zg, st = e.lanczos(1, want_vectors=True)
        assert st["vectors_saved"] == save
        r = oracle.spmv_acc(A, np.zeros_like(zg[0]), zg[0]) - eg[0] * zg[0]
        assert np.linalg.norm(r) < 1e-5


@pytest.mark.parametrize("name", ["hubbard", "tj_complex"])
def test_reortho_and_excited_states(mats, name):
    A = mats[name]
    dt = "c128" if A.is_complex else "f64"
    init = oracle.fill_random(A.nrows, 1234, A.is_complex)
    dense = np.linalg.eigvalsh(A.to_scipy().toarray())
    eo, _, so = oracle.lanczos_solve(A, init, nstates=3, max_steps=150, eps=1e-13, reortho=True)
    with LanczosEngine(dtype=dt, reortho=True, max_steps=150, eps=1e-13) as e:
        e.set_csr(A.rowptr, A.colind, A.values)
        eg, zg, st = e.lanczos(3, want_vectors=True)
        assert abs(eg[0] - dense[0]) <= E_TOL * abs(dense[0])
        assert rel(eg, eo) < 1e-8
        # with full re-orthogonalisation the Krylov basis stays orthonormal: Ritz vectors are orthonormal
        G = zg.conj() @ zg.T
        assert np.abs(G - np.eye(3)).max() < 1e-8


def test_device_assembly_is_bit_exact():
    L = 8
    hop = square(2, 4, -1.0, pbc=False) + 0.0
    U = np.linspace(1.0, 4.5, L)
    V = np.linspace(-0.5, 0.5, 2 * L)
    A = oracle.hubbard_csr(L, 3, 4, hop, U, V)
    with LanczosEngine() as e:
        e.assemble_hubbard(L, 3, 4, hop, U, V)
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind)
        assert np.array_equal(va.view(np.uint64), A.values.view(np.uint64))
    # complex hoppings
    hc = chain(6, -1.0).astype(complex)
    hc[2, 3] = -0.7 * np.exp(0.4j)
    hc[3, 2] = np.conj(hc[2, 3])
    A = oracle.hubbard_csr(6, 2, 3, hc, np.full(6, 3.0))
    with LanczosEngine(dtype="c128") as e:
        e.assemble_hubbard(6, 2, 3, hc, np.full(6, 3.0))
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind)
        assert np.array_equal(va.view(np.uint64), A.values.view(np.uint64))
    # Heisenberg ring with field
    L = 12
    jpm, jzz = chain(L, 1.0, True), chain(L, 0.7, True)
    jpm[0, 5] = jpm[5, 0] = 0.3
    field = np.linspace(-0.2, 0.2, L)
    A = oracle.heis_csr(L, 1, 5, jpm, jzz, field=field, literal_index=True)
    with LanczosEngine() as e:
        e.assemble_heisenberg(L, 5, jpm, jzz, field)
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind)
        assert np.array_equal(va.view(np.uint64), A.values.view(np.uint64))
    # t-J, complex engine, real couplings (config 4 style) and potential
    L = 8
    pv = np.linspace(-0.1, 0.2, 2 * L)
    A = oracle.tj_csr(L, 3, 2, square(2, 4, -1.0, False), square(2, 4, 0.4, False), square(2, 4, 0.4, False),
                      square(2, 4, -0.1, False), potentialV=pv, force_complex=True, literal_index=True)
    with LanczosEngine(dtype="c128") as e:
        e.assemble_tj(L, 3, 2, square(2, 4, -1.0, False), square(2, 4, 0.4, False), square(2, 4, 0.4, False),
                      square(2, 4, -0.1, False), pv)
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind)
        assert np.array_equal(va.view(np.uint64), A.values.view(np.uint64))


def test_config1_hubbard_chain_L12():
    """BASELINE config 1 shape (N=853,776; Z=11,099,088): device assembly == oracle assembly, energy parity."""
    L = 12
    hop, U = chain(L, -1.0), np.full(L, 4.0)
    A = oracle.hubbard_csr(L, 6, 6, hop, U)
    assert (A.nrows, A.nnz) == (853776, 11099088)
    eo, _, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234), want_vectors=False, nthreads=0)
    with LanczosEngine() as e:
        e.assemble_hubbard(L, 6, 6, hop, U)
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind) and np.array_equal(va, A.values)
        eg, _, st = e.lanczos(1, want_vectors=False)
        assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0])
        assert st["steps"] == so


def test_input0_free_fermions():
    """TestSuite/inputs/input0.inp parameters: L=4 OBC, t=-1, U=0, 2 up 2 down -> E0 = -2 sqrt(5)."""
    with LanczosEngine() as e:
        e.assemble_hubbard(4, 2, 2, chain(4, -1.0), np.zeros(4))
        assert e.rows() == 36
        eg, _, _ = e.lanczos(1)
        assert abs(eg[0] + 2 * np.sqrt(5)) < 1e-12


@pytest.mark.parametrize("case", ["chain_real", "square_complex", "tiny", "no_window", "beyond_lds_real", "beyond_lds_complex"])
def test_matrix_free_hubbard_matches_stored_and_otf(case, monkeypatch):
    """N1: the on-the-fly (Kronecker) product equals the stored product and the oracle's restatement of
    HubbardHelper::matrixVectorProduct; the Lanczos solve on it matches the oracle energy to 1e-10."""
    if case == "chain_real":
        L, nup, ndown = 10, 5, 4
        hop, U, V = chain(L, -1.0, True), np.linspace(2.0, 5.0, L), np.linspace(-0.4, 0.4, 2 * L)
    elif case == "square_complex":
        L, nup, ndown = 8, 3, 4
        hop = square(2, 4, -1.0, False).astype(complex)
        hop[0, 1] *= np.exp(0.3j)
        hop[1, 0] = np.conj(hop[0, 1])
        U, V = np.full(L, 4.0), np.zeros(2 * L)
    elif case == "tiny":
        L, nup, ndown = 4, 2, 2
        hop, U, V = chain(L, -1.0), np.zeros(L), np.zeros(2 * L)
    elif case == "beyond_lds_real":
        # N_up = C(18,9) = 48620 doubles exceed the LDS window: the source row is staged in three pieces
        L, nup, ndown = 18, 9, 1
        hop, U, V = square(3, 6, -1.0, True), np.full(L, 4.0), np.linspace(-0.2, 0.2, 2 * L)
    elif case == "beyond_lds_complex":
        L, nup, ndown = 16, 8, 1  # 12870 complex elements: two pieces
        hop = square(4, 4, -1.0, True).astype(complex)
        hop[0, 1] *= np.exp(0.3j)
        hop[1, 0] = np.conj(hop[0, 1])
        U, V = np.full(L, 4.0), np.zeros(2 * L)
    else:
        monkeypatch.setenv("LPP_KRON_NO_WINDOW", "1")
        L, nup, ndown = 9, 4, 4
        hop, U, V = chain(L, -1.0, True), np.full(L, 3.0), np.linspace(0, 0.3, 2 * L)
    A = oracle.hubbard_csr(L, nup, ndown, hop, U, V)
    dt = "c128" if A.is_complex else "f64"
    x0 = oracle.fill_random(A.nrows, 7, A.is_complex)
    y = oracle.fill_random(A.nrows, 8, A.is_complex)
    xo = oracle.spmv_acc(A, x0.copy(), y)
    with LanczosEngine(dtype=dt) as e:
        e.setup_hubbard_onthefly(L, nup, ndown, hop, U, V)
        assert e.rows() == A.nrows
        xg = e.matrixVectorProduct(x0.copy(), y)
        assert rel(xg, xo) < SPMV_TOL
        if not A.is_complex:
            xf = x0.copy()
            oracle.hubbard_otf_mvp(L, nup, ndown, hop, U, V, xf, y, 0, 0, 2)
            assert rel(xg, xf) < SPMV_TOL
        with pytest.raises(LppError):
            e.get_csr()
        eo, _, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234, A.is_complex), want_vectors=False)
        eg, zg, st = e.lanczos(1, want_vectors=True)
        assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0])
        # same stopping step; the 160-step runs of the big one-species spaces may cross eps one step apart (rounding)
        assert abs(st["steps"] - so) <= (1 if case.startswith("beyond_lds") else 0)
        r = oracle.spmv_acc(A, np.zeros_like(zg[0]), zg[0]) - eg[0] * zg[0]
        # residual of the Ritz vector: ~sqrt(eps) of the energy criterion; the 160-step runs on (near-)degenerate
        # one-hole spectra end a little higher
        assert np.linalg.norm(r) < (1e-3 if case.startswith("beyond_lds") else 1e-5)
        assert st["nnz"] == A.nnz  # the equivalent stored CSR has exactly the oracle's entries
    if case == "tiny":
        assert abs(eg[0] + 2 * np.sqrt(5)) < 1e-12


@pytest.mark.parametrize("name", ["hubbard", "tj_complex"])
def test_scale_free_recurrence_equals_normalised(mats, name, monkeypatch):
    """The scale-free form (unnormalised Lanczos vectors, no swap pass) yields the same tridiagonal matrix."""
    A = mats[name]
    dt = "c128" if A.is_complex else "f64"
    init = oracle.fill_random(A.nrows, 1234, A.is_complex)
    with LanczosEngine(dtype=dt, max_steps=60, eps=0.0, save_vectors=0) as e:
        e.set_csr(A.rowptr, A.colind, A.values)
        a1, b1, _ = e.decomposition(init)
        monkeypatch.setenv("LPP_NO_SCALE_FREE", "1")
        a2, b2, _ = e.decomposition(init)
        monkeypatch.delenv("LPP_NO_SCALE_FREE")
        assert len(a1) == len(a2) == 60
        assert rel(a1[:40], a2[:40]) < 1e-9 and rel(b1[:40], b2[:40]) < 1e-9
        # incremental interface reports the same coefficients
        e.begin(init)
        e.step(25)
        e.sync()
        a3, b3 = e.coeffs()
        assert rel(a3, a1[:25]) < 1e-12 and rel(b3, b1[:25]) < 1e-12
        # two-pass Ritz vector (scale-free second pass) is an eigenvector
    with LanczosEngine(dtype=dt, save_vectors=0) as e:
        e.set_csr(A.rowptr, A.colind, A.values)
        eg, zg, st = e.lanczos(1, init=init, want_vectors=True)
        assert st["vectors_saved"] == 0
        r = oracle.spmv_acc(A, np.zeros_like(zg[0]), zg[0]) - eg[0] * zg[0]
        assert np.linalg.norm(r) < 1e-5 and abs(np.linalg.norm(zg[0]) - 1) < 1e-8


def test_matrix_free_with_reortho_and_excited_states():
    """The matrix-free product under the vector-keeping (normalised) recurrence: reortho, 3 lowest states.
    Excited= semantics (Engine.h:601-657 -> LanczosSolver::computeAllStatesBelow): the run stops when the GROUND state has
    converged, the excited Ritz pairs are whatever the Krylov space holds at that step -- so the contract is: the same
    stopping step and the same three Ritz values as the oracle's run of the same loop (1e-8), not the exact levels."""
    L, nup, ndown = 8, 4, 3
    hop, U = chain(L, -1.0, True), np.full(L, 4.0)
    A = oracle.hubbard_csr(L, nup, ndown, hop, U)
    dense = np.linalg.eigvalsh(A.to_scipy().toarray())
    # eps above the rounding floor of the energy differences, so that both runs cross it at the same step
    eo, zo, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234), nstates=3, max_steps=150, eps=1e-11, reortho=True)
    with LanczosEngine(reortho=True, max_steps=150, eps=1e-11) as e:
        e.setup_hubbard_onthefly(L, nup, ndown, hop, U)
        eg, zg, st = e.lanczos(3, want_vectors=True)
    assert st["steps"] == so
    assert abs(eg[0] - dense[0]) <= E_TOL * abs(dense[0])
    assert rel(eg, eo) < 1e-8
    assert np.abs(zg @ zg.T - np.eye(3)).max() < 1e-8
    r = oracle.spmv_acc(A, np.zeros_like(zg[0]), zg[0]) - eg[0] * zg[0]
    assert np.linalg.norm(r) < 1e-5
    # Ritz values are variational: never below the exact levels a single start vector can see
    lev = np.unique(np.round(dense, 8))
    assert np.all(eg[1:] >= lev[1:3] - 1e-7)
    # and each Ritz pair has the residual of the oracle's pair (same Krylov space)
    for k in range(3):
        rg = np.linalg.norm(oracle.spmv_acc(A, np.zeros_like(zg[k]), zg[k]) - eg[k] * zg[k])
        ro = np.linalg.norm(oracle.spmv_acc(A, np.zeros_like(zo[k]), zo[k]) - eo[k] * zo[k])
        assert abs(rg - ro) <= 1e-6 + 1e-3 * ro, (k, rg, ro)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("case", ["hubbard_window", "hubbard_uniform_window", "hubbard_sliced", "hubbard_complex_window", "tj_sliced"])
def test_shared_offset_layout_is_lossless(case):
    """Entries shared by all rows of a slice are stored once per slice (and, in the window kernel, per-row columns as
    16-bit block-local indices): SpMV parity and a bit-exact get_csr round trip through the compressed layout."""
    if case.startswith("hubbard"):
        L, nu, nd = 12, 6, 3
        cplx = "complex" in case
        hop = chain(L, -1.0, True).astype(complex if cplx else float)
        if cplx:
            hop[0, 1] = -1.0 * np.exp(0.3j)
            hop[1, 0] = np.conj(hop[0, 1])
        if "uniform" in case:  # few distinct values: dictionary codes, and with them the block-periodic column template
            A = oracle.hubbard_csr(L, nu, nd, hop, np.full(L, 4.0))
        else:
            A = oracle.hubbard_csr(L, nu, nd, hop, np.linspace(1.0, 4.0, L), np.linspace(-0.3, 0.3, 2 * L))
        block = 924  # N_up = C(12,6): >= 512 rows, so the window kernel takes one basis block per window
    else:
        L = 10
        A = oracle.tj_csr(L, 4, 3, chain(L, -1.0), chain(L, 0.4), chain(L, 0.4), chain(L, -0.1), force_complex=True)
        block = 0
    kernel = 3 if case.endswith("window") else 2
    with LanczosEngine(dtype="c128" if A.is_complex else "f64", spmv_kernel=kernel) as e:
        e.set_row_block(block)
        e.set_csr(A.rowptr, A.colind, A.values)
        lay = e.layout()
        assert lay["nnz"] == A.rowptr[-1]
        assert lay["kernel"] == kernel
        if case.startswith("hubbard"):
            # every down-hop is shared; with the window kernel the per-row rest is block-local
            assert lay["shared_entries"] > 0 and lay["per_row_entries"] < 0.7 * lay["nnz"]
            assert lay["local16"] == (1 if kernel == 3 else 0)
            if kernel == 3:
                assert lay["rows_per_block"] == block
                # every block of the product basis repeats block 0's in-block structure (it is H_up); the template
                # needs the value codes (site-dependent U and V give more than 256 distinct diagonal values)
                assert lay["block_template"] == 2 * lay["coded"] and lay["diagonal_codes"] == lay["coded"]
                assert lay["coded"] == (1 if "uniform" in case else 0)
        x0 = oracle.fill_random(A.nrows, 7, A.is_complex)
        y = oracle.fill_random(A.nrows, 8, A.is_complex)
        assert rel(e.matrixVectorProduct(x0.copy(), y), oracle.spmv_acc(A, x0.copy(), y)) < SPMV_TOL
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind)
        assert np.array_equal(_bits(va), _bits(A.values))
        eg = e.computeAllStatesBelow(1, want_vectors=False)[0][0]
    eo = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234, A.is_complex), 1, want_vectors=False)[0][0]
    assert abs(eg - eo) <= E_TOL * abs(eo)


def test_unsorted_rows_keep_their_order():
    """The shared-offset split needs sorted rows; an unsorted CSR must still multiply correctly and come back from
    get_csr in exactly the order it was given."""
    A = oracle.hubbard_csr(8, 4, 4, chain(8, -1.0), np.full(8, 4.0))
    rng = np.random.default_rng(5)
    ci = A.colind.copy()
    va = A.values.copy()
    for r in range(A.nrows):
        p0, p1 = A.rowptr[r], A.rowptr[r + 1]
        perm = rng.permutation(p1 - p0)
        ci[p0:p1] = ci[p0:p1][perm]
        va[p0:p1] = va[p0:p1][perm]
    with LanczosEngine(spmv_kernel=2) as e:
        e.set_csr(A.rowptr, ci, va)
        assert e.layout()["shared_entries"] == 0
        x0 = oracle.fill_random(A.nrows, 7)
        y = oracle.fill_random(A.nrows, 8)
        assert rel(e.matrixVectorProduct(x0.copy(), y), oracle.spmv_acc(A, x0.copy(), y)) < SPMV_TOL
        rp, c2, v2 = e.get_csr()
        assert np.array_equal(c2, ci) and np.array_equal(_bits(v2), _bits(va))


@pytest.mark.parametrize("cplx", [False, True])
def test_shared_offsets_beyond_the_per_slice_capacity(cplx):
    """A Toeplitz band with 81 diagonals: every entry is shared by all rows of a slice, but a slice holds at most 64
    shared entries; the rest must stay per-row entries.  Rows near the edges are shorter (ragged slices), the last
    slice is partial."""
    n, hb = 1000, 40
    rng = np.random.default_rng(11)
    dv = rng.standard_normal(2 * hb + 1) + (1j * rng.standard_normal(2 * hb + 1) if cplx else 0)
    rowptr, ci, va = [0], [], []
    for r in range(n):
        for d in range(-hb, hb + 1):
            c = r + d
            if 0 <= c < n:
                ci.append(c)
                va.append(dv[d + hb])
        rowptr.append(len(ci))
    A = oracle.Csr(np.array(rowptr, np.int64), np.array(ci, np.int32), np.array(va, complex if cplx else float))
    with LanczosEngine(dtype="c128" if cplx else "f64", spmv_kernel=2) as e:
        e.set_csr(A.rowptr, A.colind, A.values)
        lay = e.layout()
        assert lay["shared_stride"] == 64 and 0 < lay["per_row_entries"] < lay["nnz"]
        x0 = oracle.fill_random(n, 7, cplx)
        y = oracle.fill_random(n, 8, cplx)
        assert rel(e.matrixVectorProduct(x0.copy(), y), oracle.spmv_acc(A, x0.copy(), y)) < SPMV_TOL
        rp, c2, v2 = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(c2, A.colind) and np.array_equal(_bits(v2), _bits(A.values))


def test_engine_reuse_across_matrices_and_engines():
    """One engine takes a sequence of different matrices (device-assembled, uploaded with and without a row-block hint,
    matrix-free) and every product / solve is right; a second engine alive at the same time does not disturb it."""
    L = 10
    hop = chain(L, -1.0, True)
    H1 = oracle.hubbard_csr(L, 5, 5, hop, np.full(L, 4.0))          # N_up = 252
    H2 = oracle.heis_csr(14, 1, 7, chain(14, 1.0), chain(14, 1.0))  # other size, no block structure
    H3 = oracle.hubbard_csr(8, 4, 3, chain(8, -1.0), np.linspace(1, 3, 8))

    def check(e, A):
        x0, y = oracle.fill_random(A.nrows, 3), oracle.fill_random(A.nrows, 4)
        assert rel(e.matrixVectorProduct(x0.copy(), y), oracle.spmv_acc(A, x0.copy(), y)) < SPMV_TOL
        eo = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234), want_vectors=False)[0][0]
        eg = e.computeAllStatesBelow(1, want_vectors=False)[0][0]
        assert abs(eg - eo) <= E_TOL * abs(eo)

    with LanczosEngine(max_steps=300) as e, LanczosEngine(max_steps=300) as other:
        other.assemble_heisenberg(12, 6, chain(12, 1.0, True), chain(12, 1.0, True))
        e.assemble_hubbard(L, 5, 5, hop, np.full(L, 4.0))
        check(e, H1)
        e.set_csr(H2.rowptr, H2.colind, H2.values)                  # smaller matrix, hint still 0
        check(e, H2)
        e.set_row_block(252)
        e.set_csr(H1.rowptr, H1.colind, H1.values)                  # uploaded with the basis block
        check(e, H1)
        e.setup_hubbard_onthefly(L, 5, 5, hop, np.full(L, 4.0))     # matrix-free on the same engine
        check(e, H1)
        e.set_row_block(0)
        e.set_csr(H3.rowptr, H3.colind, H3.values)
        check(e, H3)
        a, b, st = e.decomposition()
        assert st["steps"] >= 4 and len(a) == len(b) == st["steps"]
        rp, ci, va = other.get_csr()
        O = oracle.heis_csr(12, 1, 6, chain(12, 1.0, True), chain(12, 1.0, True), literal_index=True)
        assert np.array_equal(rp, O.rowptr) and np.array_equal(ci, O.colind) and np.array_equal(_bits(va), _bits(O.values))


def _random_structured_csr(rng, cplx, product_like=False):
    """Random matrices that exercise the layout machinery: a block-periodic in-block pattern (sometimes perturbed in one
    block), block-shifted couplings shared by all rows of a block (sometimes broken in one row), a diagonal that is
    present / absent / few-valued / many-valued, values from a small or a large set, last block possibly partial."""
    B = int(rng.choice([520, 576, 700])) if product_like else int(rng.choice([64, 70, 128, 200, 520, 700]))
    nblocks = int(rng.integers(2, 9))
    n = B * nblocks - (int(rng.integers(0, B // 2)) if (rng.random() < 0.3 and not product_like) else 0)
    few = True if product_like else rng.random() < 0.7
    pool = rng.standard_normal(4) if few else None

    def value():
        v = rng.choice(pool) if few else rng.standard_normal()
        if cplx:
            v = v + 1j * (rng.choice(pool) if few else rng.standard_normal())
        return v

    local = {}  # block-periodic pattern: local row -> {local col: value}
    for r in range(B):
        cols = rng.choice(B, size=int(rng.integers(0, 7)), replace=False)
        local[r] = {int(c): value() for c in cols if c != r}
    shifts = {int(k): value() for k in rng.choice(np.arange(-3, 4), size=int(rng.integers(0, 5)), replace=False) if k != 0}
    diag_mode = rng.choice(["all_few", "all_few", "some", "none"]) if product_like else rng.choice(["all_few", "all_many", "some", "none"])
    rows = []
    for r in range(n):
        b, l = divmod(r, B)
        ent = {b * B + c: v for c, v in local[l].items() if b * B + c < n}
        for k, v in shifts.items():
            c = r + k * B
            if 0 <= c < n:
                ent[c] = v
        if diag_mode == "all_few":
            ent[r] = (rng.choice(pool) if few else float(rng.integers(0, 3))) + (0j if cplx else 0.0)
        elif diag_mode == "all_many":
            ent[r] = rng.standard_normal() + (0j if cplx else 0.0)
        elif diag_mode == "some" and rng.random() < 0.5:
            ent[r] = value()
        rows.append(ent)
    if rng.random() < (0.25 if product_like else 0.3):  # break the block periodicity / a shared run in one place
        r = int(rng.integers(0, n))
        c = int(rng.integers(0, n))
        rows[r][c] = value()
    if product_like and rng.random() < 0.3:  # same structure everywhere, but one in-block value differs in one block
        r = int(rng.integers(B, n))
        inblock = [c for c in rows[r] if c // B == r // B and c != r]
        if inblock:
            rows[r][inblock[0]] = rows[r][inblock[0]] * 2 + (pool[0] if few else 1.0)
    rowptr, ci, va = [0], [], []
    for ent in rows:
        for c in sorted(ent):
            ci.append(c)
            va.append(ent[c])
        rowptr.append(len(ci))
    A = oracle.Csr(np.array(rowptr, np.int64), np.array(ci, np.int32), np.array(va, complex if cplx else float))
    return A, B


@pytest.mark.parametrize("seed", range(36))
def test_layout_fuzz_spmv_and_roundtrip(seed):
    rng = np.random.default_rng(1000 + seed)
    cplx = bool(seed % 3 == 2)
    product_like = seed >= 12  # block-periodic with a basis block >= 512 rows and few values: template, diagonal codes
    A, B = _random_structured_csr(rng, cplx, product_like)
    if A.nnz == 0:
        pytest.skip("empty draw")
    kernel = 3 if product_like else [2, 3, 3][seed % 3]
    hint = B if (kernel == 3 and (product_like or rng.random() < 0.8)) else 0
    with LanczosEngine(dtype="c128" if cplx else "f64", spmv_kernel=kernel) as e:
        e.set_row_block(hint)
        e.set_csr(A.rowptr, A.colind, A.values)
        x0 = oracle.fill_random(A.nrows, 7, cplx)
        y = oracle.fill_random(A.nrows, 8, cplx)
        xo = oracle.spmv_acc(A, x0.copy(), y)
        xg = e.matrixVectorProduct(x0.copy(), y)
        assert np.max(np.abs(xg - xo)) <= 1e-12 * max(1.0, np.max(np.abs(xo))), e.layout()
        rp, c2, v2 = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(c2, A.colind) and np.array_equal(_bits(v2), _bits(A.values)), e.layout()


def _hip_runtime():
    """The HIP runtime instance the engine itself is linked against (found in this process' maps once the engine library is
    loaded): torch would bring its own copy of the runtime, and two of them in one process do not share a device."""
    import ctypes as C
    from lanczosplusplus_amd import _capi
    _capi.lib()
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not mapped")


def test_set_csr_from_device_pointers():
    """lpp_engine_set_csr_device: a CSR that already lives on the GPU gives the same layout, product and round trip as the
    host upload; a malformed one is refused."""
    import ctypes as C
    A = oracle.hubbard_csr(10, 5, 4, chain(10, -1.0, True), np.full(10, 4.0))
    with LanczosEngine(spmv_kernel=3) as e, LanczosEngine(spmv_kernel=3) as h:
        hip = _hip_runtime()
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]

        def to_device(a):
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), a.nbytes) == 0
            assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0  # hipMemcpyHostToDevice
            return p

        rp, ci, va = to_device(A.rowptr), to_device(A.colind), to_device(A.values)
        bad_ci = A.colind.copy()
        bad_ci[5] = A.nrows  # column out of range
        bad = to_device(bad_ci)
        try:
            e.set_row_block(252)
            e.set_csr_device(A.nrows, rp.value, ci.value, va.value)
            h.set_row_block(252)
            h.set_csr(A.rowptr, A.colind, A.values)
            assert e.layout() == h.layout()
            x0, y = oracle.fill_random(A.nrows, 3), oracle.fill_random(A.nrows, 4)
            assert rel(e.matrixVectorProduct(x0.copy(), y), oracle.spmv_acc(A, x0.copy(), y)) < SPMV_TOL
            r2, c2, v2 = e.get_csr()
            assert np.array_equal(r2, A.rowptr) and np.array_equal(c2, A.colind) and np.array_equal(_bits(v2), _bits(A.values))
            with pytest.raises(LppError):
                e.set_csr_device(A.nrows, rp.value, bad.value, va.value)
        finally:
            for p in (rp, ci, va, bad):
                hip.hipFree(p)


def test_basis_block_is_detected_without_a_hint():
    """An uploaded product-basis matrix that nobody described gets the same layout as a hinted one: the basis block is
    read off the structure (couplings at multiples of N_up shared by 64 consecutive rows).  Matrices without such a
    structure are left alone."""
    L = 12
    A = oracle.hubbard_csr(L, 6, 5, chain(L, -1.0, True), np.full(L, 4.0))  # N_up = 924, N = 731,808
    with LanczosEngine() as auto, LanczosEngine() as hinted:
        auto.set_csr(A.rowptr, A.colind, A.values)
        hinted.set_row_block(924)
        hinted.set_csr(A.rowptr, A.colind, A.values)
        la, lh = auto.layout(), hinted.layout()
        assert la["rows_per_block"] == 924 and la == lh and la["block_template"] == 2
        x0, y = oracle.fill_random(A.nrows, 3), oracle.fill_random(A.nrows, 4)
        assert rel(auto.matrixVectorProduct(x0.copy(), y), oracle.spmv_acc(A, x0.copy(), y)) < SPMV_TOL
    H = oracle.heis_csr(22, 1, 11, chain(22, 1.0), chain(22, 1.0))  # 705,432 states, no uniform block
    with LanczosEngine() as e:
        e.set_csr(H.rowptr, H.colind, H.values)
        assert e.layout()["rows_per_block"] != 924 and e.layout()["block_template"] == 0
        x0, y = oracle.fill_random(H.nrows, 3), oracle.fill_random(H.nrows, 4)
        assert rel(e.matrixVectorProduct(x0.copy(), y), oracle.spmv_acc(H, x0.copy(), y)) < SPMV_TOL


@pytest.mark.parametrize("source", ["assembled", "uploaded"])
def test_split_panel_layout_of_a_plain_format_matrix(source, monkeypatch):
    """Plain-format matrix (no value dictionary, no shared offsets) with a basis block: the entries that leave the row blocks are
    held in a second CSR whose rows are panel-major (16 positions of every block, then the next 16) and applied by a second
    launch through a row map.  Same bytes per entry as the CSR; get_csr merges the two parts back bit for bit; products and
    energies as before.  Real matrices (complex ones keep the sliced kernel and are checked to be left alone)."""
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "0")
    monkeypatch.setenv("LPP_COMPRESS_VALUES", "0")
    monkeypatch.setenv("LPP_SHARED_OFFSETS", "0")
    monkeypatch.setenv("LPP_SPLIT_PANEL", "1")  # opt-in layout (bench.py's plain-format leg takes it)
    monkeypatch.setenv("LPP_SPLIT_PARTS", "3")  # several source-range parts forced onto the small matrix
    for dt in ("f64", "c128"):
        L, nup, ndown = 12, 6, 5
        hop = chain(L, -1.0, True).astype(complex if dt == "c128" else float)
        if dt == "c128":
            hop[0, 1] *= np.exp(0.3j)
            hop[1, 0] = np.conj(hop[0, 1])
        U, V = np.linspace(2.0, 4.0, L), np.linspace(-0.3, 0.3, 2 * L)
        A = oracle.hubbard_csr(L, nup, ndown, hop, U, V)
        x0, y = oracle.fill_random(A.nrows, 7, A.is_complex), oracle.fill_random(A.nrows, 8, A.is_complex)
        xo = oracle.spmv_acc(A, x0.copy(), y)
        eo, _, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234, A.is_complex), want_vectors=False)
        with LanczosEngine(dtype=dt) as e:
            if source == "assembled":
                e.assemble_hubbard(L, nup, ndown, hop, U, V)
            else:
                e.set_row_block(comb(L, nup))
                e.set_csr(A.rowptr, A.colind, A.values)
            lay = e.layout()
            assert lay["coded"] == 0 and lay["nnz"] == A.nnz
            if dt == "f64":
                assert lay["kernel"] == 3 and lay["split_panel"] >= 1 and lay["rows_per_block"] == comb(L, nup)
            else:  # complex matrices keep the sliced kernel (16-byte window elements lose): nothing to split
                assert lay["kernel"] == 2 and lay["split_panel"] == 0
            assert e.stats()["nnz"] == A.nnz
            rp, ci, va = e.get_csr()
            assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind)
            assert np.array_equal(np.ascontiguousarray(va).view(np.uint64), np.ascontiguousarray(A.values).view(np.uint64))
            assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL
            eg, zg, st = e.lanczos(1, want_vectors=True)
            assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0]) and st["steps"] == so
            r = oracle.spmv_acc(A, np.zeros_like(zg[0]), zg[0]) - eg[0] * zg[0]
            assert np.linalg.norm(r) < 1e-5
        monkeypatch.setenv("LPP_SPLIT_PANEL", "0")
        with LanczosEngine(dtype=dt) as e:
            e.assemble_hubbard(L, nup, ndown, hop, U, V)
            assert e.layout()["split_panel"] == 0
            assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL
        monkeypatch.setenv("LPP_SPLIT_PANEL", "1")


def test_uploaded_csr_takes_the_product_basis_layout(monkeypatch):
    """The reference hands its Hamiltonian over as a CSR (DefaultSymmetry.h:54-57 -> InternalProductStored.h:116).  A Hubbard CSR
    uploaded through lpp_engine_set_csr -- no hint, no model knowledge -- ends in the same product-basis layout device assembly
    builds: the basis block is detected, T, C and D are read off the matrix and EVERY row of the CSR is verified against them
    before the CSR is dropped.  get_csr gives the uploaded arrays back bit for bit; one changed value anywhere keeps the general layout."""
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")  # below the size from which the layout is chosen by itself
    for case in ("chain_L12", "disorder"):
        L, nup, ndown, hop, U, V = PB_CASES[case]()
        A = oracle.hubbard_csr(L, nup, ndown, hop, U, V)
        x0, y = oracle.fill_random(A.nrows, 7), oracle.fill_random(A.nrows, 8)
        xo = oracle.spmv_acc(A, x0.copy(), y)
        eo, _, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234), want_vectors=False)
        with LanczosEngine() as e, LanczosEngine() as d:
            e.set_csr(A.rowptr, A.colind, A.values)
            d.assemble_hubbard(L, nup, ndown, hop, U, V)
            lay = e.layout()
            assert lay["kernel"] == 4 and lay == d.layout(), (lay, d.layout())
            assert lay["diagonal_plain"] == (1 if case == "disorder" else 0)
            rp, ci, va = e.get_csr()
            assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind) and np.array_equal(_bits(va), _bits(A.values))
            assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL
            eg, _, st = e.lanczos(1, want_vectors=False)
            assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0]) and st["steps"] == so
            e.set_row_block(comb(L, nup))  # the shim's hint (BasisHubbardLanczos::sizeUp()): same result without the detection
            e.set_csr(A.rowptr, A.colind, A.values)
            assert e.layout() == lay
        # not a product-basis matrix any more: one off-diagonal value of one row in the middle differs from its template
        B = oracle.Csr(A.rowptr.copy(), A.colind.copy(), A.values.copy())
        r = A.nrows // 2 + 17
        k = A.rowptr[r] + (0 if A.colind[A.rowptr[r]] != r else 1)
        B.values[k] *= 1.5
        with LanczosEngine() as e:
            e.set_csr(B.rowptr, B.colind, B.values)
            assert e.layout()["kernel"] != 4
            rp, ci, va = e.get_csr()
            assert np.array_equal(ci, B.colind) and np.array_equal(_bits(va), _bits(B.values))
            assert rel(e.matrixVectorProduct(x0.copy(), y), oracle.spmv_acc(B, x0.copy(), y)) < SPMV_TOL


PB_CASES = {
    # name: (L, nup, ndown, hop, U, V)   -- N_up >= 512 so that device assembly takes the product-basis layout
    "chain_L12": lambda: (12, 6, 5, chain(12, -1.0, True), np.where(np.arange(12) % 3 == 0, 2.0, 4.0), np.tile([0.25, -0.5, 0.0], 8)),
    "ladder_2x6": lambda: (12, 6, 6, square(2, 6, -1.0, True), np.full(12, 4.0), np.zeros(24)),
    "open_chain_L12": lambda: (12, 6, 6, chain(12, -1.0, False), np.full(12, 4.0), np.zeros(24)),  # one value group (no sign changes); a_j > b_j
    "two_hoppings": lambda: (12, 5, 7, chain(12, -1.0, False) + 0.5 * (np.diag(np.ones(10), 2) + np.diag(np.ones(10), -2)), np.full(12, 3.0), np.zeros(24)),
    # site-dependent U and potentials (HubbardHelper.h:138-189 with disorder): thousands of distinct diagonal values -- the diagonal
    # travels as a plain f64 stream added by the streaming pass, T and C are unchanged
    "disorder": lambda: (12, 6, 5, chain(12, -1.0, True), np.random.default_rng(5).uniform(1, 5, 12), np.random.default_rng(6).uniform(-0.5, 0.5, 24)),
}


_PB_ORACLE = {}


def _pb_oracle(case):
    """the oracle's side of test_product_basis_layout, once per case (its five forms compare against the same numbers)"""
    if case not in _PB_ORACLE:
        L, nup, ndown, hop, U, V = PB_CASES[case]()
        A = oracle.hubbard_csr(L, nup, ndown, hop, U, V)
        x0, y = oracle.fill_random(A.nrows, 7), oracle.fill_random(A.nrows, 8)
        xo = oracle.spmv_acc(A, x0.copy(), y)
        init = oracle.fill_random(A.nrows, 4321)
        eo, zo, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234), nstates=1)
        steps_o, ao, bo, _, _ = oracle.lanczos_decomposition(A, init)
        e3o, _, s3o = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234), nstates=3, max_steps=150, eps=1e-11, reortho=True)
        _PB_ORACLE.clear()  # one case at a time (the parametrisation runs a case's forms back to back)
        _PB_ORACLE[case] = (A, x0, y, xo, init, eo, so, steps_o, ao, bo, e3o, s3o)
    return _PB_ORACLE[case]


@pytest.mark.parametrize("form", ["window", "natural", "segments", "pieces", "wide", "wide_rounds"])
@pytest.mark.parametrize("case", sorted(PB_CASES))
def test_product_basis_layout(case, form, monkeypatch):
    """Device assembly of Hubbard straight into the product-basis layout (T, C, diagonal codes; lpp_pb_kernels.h): the CSR it
    stands for is the oracle's bit for bit, x += H y (two kernels, pitched vectors) matches the oracle, and every solver entry
    point works on the pitched vectors; the general layout (LPP_PRODUCT_LAYOUT=0) gives the same numbers.
    form "pieces": the kernels for rows beyond one LDS window and vectors beyond 4 GiB (lpp_pbig_kernels.h: BASELINE config 5's
    sectors) forced onto the same small matrices -- rows cut into pieces of 256 positions (entries that leave a piece are read
    from memory), couplings over 3 parts of the source range with 64-bit addresses; "wide": pieces of 320 positions and the
    whole-panel coupling kernel with 64-bit addresses (what BASELINE config 5's sectors take on one GPU); "segments": what those
    sectors take since round 4 -- the in-block matrix decomposed by the high sites of the species' basis word (lpp_pbseg.h, k_pb_up_seg:
    segments of <= 256 positions here), read off T and verified against it; a species with more than two hopping magnitudes
    (two_hoppings) keeps the per-position template; "wide_rounds" (round 5): "wide" with every workgroup of the coupling kernel walking its
    block range in two pieces per panel, one LDS image of coupling lists each (what sectors of 65536 blocks and more take)."""
    L, nup, ndown, hop, U, V = PB_CASES[case]()
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")  # these matrices are below the size from which the layout is chosen by itself
    if form in ("pieces", "segments"):
        monkeypatch.setenv("LPP_PB_PIECE_ROWS", "256")
        monkeypatch.setenv("LPP_PB_PARTS", "3")
        monkeypatch.setenv("LPP_PB_SEG", "1" if form == "segments" else "0")  # "pieces": the per-position template (k_pb_up_big2)
    if form == "natural":
        monkeypatch.setenv("LPP_PB_PERM", "0")  # positions of a block in the basis order ("window": stored in the order of their list lengths)
    if form == "wide_rounds":
        monkeypatch.setenv("LPP_PB_DOWN_ROUNDS", "2")
        if case in ("chain_L12", "disorder"):
            monkeypatch.setenv("LPP_PB_DOWN_IMAGE", "0")  # the round's image rebuilt from the coupling lists instead of copied from the prepared buffer
    if form in ("wide", "wide_rounds"):
        monkeypatch.setenv("LPP_PB_PIECE_ROWS", "320")
        monkeypatch.setenv("LPP_PB_WIDE", "1")
        monkeypatch.setenv("LPP_PB_BIG2", "0")  # one block per workgroup (k_pb_up_big); "pieces" runs two per workgroup (k_pb_up_big2)
    A, x0, y, xo, init, eo, so, steps_o, ao, bo, e3o, s3o = _pb_oracle(case)
    with LanczosEngine() as e:
        e.assemble_hubbard(L, nup, ndown, hop, U, V)
        lay = e.layout()
        assert lay["kernel"] == 4 and lay["nnz"] == A.nnz and lay["resident_bytes"] < (0.12 if case == "disorder" else 0.05) * 12 * A.nnz
        assert (lay["diagonal_plain"], lay["diagonal_codes"], lay["chained_step"]) == ((1, 0, 0) if case == "disorder" else (0, 1, 1 if form in ("window", "natural") else 0))  # the chained step: any number of hopping values (two_hoppings: the any-number-of-groups path)
        seg = form == "segments" and case != "two_hoppings"  # C(12, 6) = 924 or C(12, 5) = 792 positions: 2 high sites, 4 segments of 210 / 252
        assert (lay["pieces"], lay["coupling_parts"]) == {"window": (1, 1), "pieces": (4, 3), "segments": (4, 3), "natural": (1, 1), "wide": (3, 1), "wide_rounds": (3, 1)}[form]
        assert lay["coupling_rounds"] == (2 if form == "wide_rounds" else 1)
        assert lay["segments"] == (4 if seg else 0)
        assert lay["rows_by_list_length"] == (1 if form == "window" else 0)  # one-window form only; internal: every check below is in the basis order
        st = e.stats()
        assert (st["nrows"], st["nnz"]) == (A.nrows, A.nnz)
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind) and np.array_equal(_bits(va), _bits(A.values))
        xg = e.matrixVectorProduct(x0.copy(), y)
        assert rel(xg, xo) < SPMV_TOL
        assert rel(e.matrixVectorProduct(xg.copy(), y) - xg, xo - x0) < 1e-12  # accumulate semantics
        eg, zg, st = e.lanczos(1, want_vectors=True)  # built-in start vector, pitched; two-pass or saved Ritz vector
        assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0]) and st["steps"] == so
        r = oracle.spmv_acc(A, np.zeros_like(zg[0]), zg[0]) - eg[0] * zg[0]
        assert np.linalg.norm(r) < 1e-5 and abs(np.linalg.norm(zg[0]) - 1) < 1e-8
        ag, bg, _ = e.decomposition(init)  # host start vector into the pitched layout
        assert len(ag) == steps_o and rel(ag, ao) < 1e-8 and rel(bg, bo) < 1e-8
        ms = e.bench_spmv(1, 2)
        assert ms > 0
        # the matrix-free entry point builds the same thing where a species' row fits the LDS window ...
        e.setup_hubbard_onthefly(L, nup, ndown, hop, U, V)
        assert e.layout()["kernel"] == 4
        assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL
        monkeypatch.setenv("LPP_ONTHEFLY_KRON", "1")  # ... and the fused block-order kernel otherwise: same product
        e.setup_hubbard_onthefly(L, nup, ndown, hop, U, V)
        with pytest.raises(LppError):
            e.layout()
        assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL
        monkeypatch.delenv("LPP_ONTHEFLY_KRON")
    with LanczosEngine(save_vectors=0) as e:  # scale-free recurrence + two-pass Ritz vector
        e.assemble_hubbard(L, nup, ndown, hop, U, V)
        eg2, zg2, st2 = e.lanczos(1, want_vectors=True)
        assert st2["vectors_saved"] == 0 and abs(eg2[0] - eo[0]) <= E_TOL * abs(eo[0])
        r = oracle.spmv_acc(A, np.zeros_like(zg2[0]), zg2[0]) - eg2[0] * zg2[0]
        assert np.linalg.norm(r) < 1e-5
    with LanczosEngine(reortho=True, max_steps=150, eps=1e-11) as e:  # blocked CGS2 on pitched Krylov columns
        e.assemble_hubbard(L, nup, ndown, hop, U, V)
        e3, z3, st3 = e.lanczos(3, want_vectors=True)
        assert st3["steps"] == s3o and rel(e3, e3o) < 1e-8
        assert np.abs(z3 @ z3.T - np.eye(3)).max() < 1e-8
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "0")
    with LanczosEngine() as e:
        e.assemble_hubbard(L, nup, ndown, hop, U, V)
        assert e.layout()["kernel"] == 3
        xw = e.matrixVectorProduct(x0.copy(), y)
        assert rel(xw, xg) < SPMV_TOL


def _pb_child(case, env, product_to=None):
    """One solve and one decomposition of a PB_CASES matrix in a child process (scale-free recurrence, LPP_PRODUCT_LAYOUT=1 plus `env`):
    (layout's chained_step, energy, steps, a, b) as a dict and the child's stderr.  product_to: also x += H y on the oracle's vectors of
    _pb_oracle, saved there."""
    import json
    import os
    import subprocess
    import sys
    code = (
        "import sys, json, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import oracle\n"
        "from test_gpu_parity import PB_CASES\n"
        "from lanczosplusplus_amd import LanczosEngine\n"
        "L, nup, ndown, hop, U, V = PB_CASES[%r]()\n"
        "with LanczosEngine(save_vectors=0) as e:\n"
        "    e.assemble_hubbard(L, nup, ndown, hop, U, V)\n"
        "    lay = e.layout()\n"
        "    n = e.stats()['nrows']\n"
        "    if len(sys.argv) > 1:\n"
        "        np.save(sys.argv[1], e.matrixVectorProduct(oracle.fill_random(n, 7), oracle.fill_random(n, 8)))\n"
        "    eg, _, st = e.lanczos(1, want_vectors=False)\n"
        "    ag, bg, _ = e.decomposition(oracle.fill_random(n, 4321))\n"
        "print('RESULT ' + json.dumps({'chained': lay['chained_step'], 'e0': float(eg[0]), 'steps': st['steps'], 'a': list(map(float, ag)), 'b': list(map(float, bg))}))\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)), case)
    env = dict(os.environ, LPP_PRODUCT_LAYOUT="1", **env)
    out = subprocess.run([sys.executable, "-c", code] + ([str(product_to)] if product_to else []), env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]), out.stderr


def test_chained_step_with_fixed_task_shares():
    """LPP_PB_DOWN_PF=0: the coupling kernel of the chained step without the task counter and without the wave that touches the u lines
    ahead (round 3's form, kept as a switch) gives the same energy, stopping step and coefficients.  The switch is read when the layout is
    built (pb_build); the run is a child process with the switch in its environment from the start."""
    case = "ladder_2x6"
    A, x0, y, xo, init, eo, so, steps_o, ao, bo, e3o, s3o = _pb_oracle(case)
    r, _ = _pb_child(case, dict(LPP_PB_DOWN_PF="0"))
    assert r["chained"] == 1
    assert abs(r["e0"] - eo[0]) <= E_TOL * abs(eo[0]) and r["steps"] == so
    assert len(r["a"]) == steps_o and rel(np.array(r["a"]), ao) < 1e-8 and rel(np.array(r["b"]), bo) < 1e-8


# ladder_2x6: 924 blocks of 924 positions on one GPU.  A panel of all blocks is 924 * 128 bytes = 116 KB (far below the 3 MB up to which the
# coupling kernels drop the pacing), a coupling workgroup owns 29 blocks (image and task sums far below 150 KB of LDS: the counter forms
# fit), and there is no exchange.  So every form is on by itself except "lazy exchange", and a switch turns off exactly its own form --
# LPP_PB_DOWN_PF=0 also "pacing dropped", which only the counter form of the chained kernel can do.
#                                          chain, down tasks, chained counter form, pacing dropped, lazy exchange
LAUNCH_FORMS = {
    "none": ({}, (1, 1, 1, 1, 0)),
    "chain0": (dict(LPP_PB_CHAIN="0"), (0, 1, 1, 1, 0)),
    "down_tasks0": (dict(LPP_PB_DOWN_TASKS="0"), (1, 0, 1, 1, 0)),
    "down_pf0": (dict(LPP_PB_DOWN_PF="0"), (1, 1, 0, 0, 0)),
    "chain_pace1": (dict(LPP_PB_CHAIN_PACE="1"), (1, 1, 1, 0, 0)),
}


@pytest.mark.parametrize("switch", list(LAUNCH_FORMS))
def test_launch_switches_select_their_forms(switch, tmp_path):
    """The product-basis launch forms are resolved once, when the layout is built (PbState::chain_ok, down_tasks, down_pf, chain_drop_pace,
    lazy_tx), and printed under LPP_VERBOSE.  Every launch switch still selects its form -- the printed line shows exactly the flags the
    environment implies, the layout reports the chained step accordingly -- and every form gives the oracle's energy, stopping step and
    coefficients (chained or three-kernel step) and the oracle's product (plain coupling kernel, which LPP_PB_DOWN_TASKS steers)."""
    import re
    case = "ladder_2x6"
    A, x0, y, xo, init, eo, so, steps_o, ao, bo, e3o, s3o = _pb_oracle(case)
    env, forms = LAUNCH_FORMS[switch]
    r, err = _pb_child(case, dict(env, LPP_VERBOSE="1"), tmp_path / "x.npy")
    lines = re.findall(r"lpp: product-basis launch forms: chain (\d+), down tasks (\d+), chained counter form (\d+), pacing dropped (\d+), lazy exchange (\d+)", err)
    print(switch, lines, r["chained"], r["e0"], r["steps"])
    assert lines and all(tuple(map(int, ln)) == forms for ln in lines), (lines, err[-2000:])
    assert r["chained"] == forms[0]
    assert rel(np.load(tmp_path / "x.npy"), xo) < SPMV_TOL
    assert abs(r["e0"] - eo[0]) <= E_TOL * abs(eo[0]) and r["steps"] == so
    assert len(r["a"]) == steps_o and rel(np.array(r["a"]), ao) < 1e-8 and rel(np.array(r["b"]), bo) < 1e-8


def test_chained_step_when_some_coupling_workgroups_own_no_block(monkeypatch):
    """364 blocks (14 sites, 3 particles of the block species) on the coupling kernel's 32 ranges of 12: the last workgroup of every
    group owns NO block (ceil(364 / 32) * 31 >= 364).  The wave of the chained step that touches the u lines ahead indexed its row table
    at -1 there (advisor finding, round 4); energy, stopping step and coefficients against the oracle."""
    L, nup, ndown = 14, 7, 3
    hop, U = chain(L, -1.0, True), np.full(L, 4.0)
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")
    A = oracle.hubbard_csr(L, nup, ndown, hop, U)
    assert A.nrows == 3432 * 364
    init = oracle.fill_random(A.nrows, 4321)
    steps_o, ao, bo, _, hist = oracle.lanczos_decomposition(A, init, nthreads=0)
    with LanczosEngine(save_vectors=0) as e:
        e.assemble_hubbard(L, nup, ndown, hop, U)
        lay = e.layout()
        assert lay["kernel"] == 4 and lay["chained_step"] == 1, lay
        ag, bg, _ = e.decomposition(init)
    assert len(ag) == steps_o and rel(ag, ao) < 1e-8 and rel(bg, bo) < 1e-8
    eg = tridiag_lowest(ag, bg[:-1], 1)[0]
    assert abs(eg - hist[-1]) <= E_TOL * abs(hist[-1])


@pytest.mark.parametrize("case", ["peierls_ring", "kane_mele_like", "disorder"])
def test_product_basis_layout_with_complex_hoppings(case, monkeypatch):
    """Complex hoppings (SolverOptions=useComplex, HubbardHelper.h:63-66; Peierls phases, KaneMele's imaginary second-neighbour hops) in the
    product-basis layout: the in-block matrix is held realified over (re, im) pairs, so k_pb_up is the real kernel, the couplings keep
    complex values (k_pb_down<CPLX>).  Same checks as the real layout test: CSR bit-exact, x += H y, solves, a/b, Ritz vector, reortho."""
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")
    L, nup, ndown = 12, 6, 5
    ring = chain(L, -1.0, True).astype(complex)
    up = np.triu(np.ones((L, L)), 1) > 0
    if case == "kane_mele_like":  # real first-neighbour hops, imaginary second-neighbour hops
        nnn = (np.diag(np.ones(L - 2), 2) + np.diag(np.ones(L - 2), -2)).astype(complex)
        hop = ring + 0.3j * np.where(up, nnn, -nnn)
    else:  # a phase on every bond
        hop = ring * np.where(up, np.exp(0.37j), np.exp(-0.37j))
    assert np.allclose(hop, hop.conj().T)
    U = np.full(L, 4.0) if case != "disorder" else np.random.default_rng(5).uniform(1, 5, L)
    V = np.zeros(2 * L) if case != "disorder" else np.random.default_rng(6).uniform(-0.5, 0.5, 2 * L)
    A = oracle.hubbard_csr(L, nup, ndown, hop, U, V)
    assert A.is_complex
    x0, y = oracle.fill_random(A.nrows, 7, True), oracle.fill_random(A.nrows, 8, True)
    xo = oracle.spmv_acc(A, x0.copy(), y)
    init = oracle.fill_random(A.nrows, 4321, True)
    eo, zo, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234, True), nstates=1)
    steps_o, ao, bo, _, _ = oracle.lanczos_decomposition(A, init)
    with LanczosEngine(dtype="c128") as e:
        e.assemble_hubbard(L, nup, ndown, hop, U, V)
        lay = e.layout()
        assert lay["kernel"] == 4 and lay["nnz"] == A.nnz and lay["rows_by_list_length"] == 0
        assert (lay["diagonal_plain"], lay["chained_step"]) == ((1, 0) if case == "disorder" else (0, 1))  # the chained pair carries complex hoppings too
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind)
        assert np.array_equal(np.ascontiguousarray(va).view(np.uint64), np.ascontiguousarray(A.values).view(np.uint64))
        xg = e.matrixVectorProduct(x0.copy(), y)
        assert rel(xg, xo) < SPMV_TOL
        eg, zg, st = e.lanczos(1, want_vectors=True)
        assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0]) and st["steps"] == so
        r = oracle.spmv_acc(A, np.zeros_like(zg[0]), zg[0]) - eg[0] * zg[0]
        assert np.linalg.norm(r) < 1e-5 and abs(np.linalg.norm(zg[0]) - 1) < 1e-8
        ag, bg, _ = e.decomposition(init)
        assert len(ag) == steps_o and rel(ag, ao) < 1e-8 and rel(bg, bo) < 1e-8
    with LanczosEngine(dtype="c128", save_vectors=0) as e:  # scale-free recurrence + two-pass Ritz vector
        e.assemble_hubbard(L, nup, ndown, hop, U, V)
        eg2, zg2, st2 = e.lanczos(1, want_vectors=True)
        assert st2["vectors_saved"] == 0 and abs(eg2[0] - eo[0]) <= E_TOL * abs(eo[0])
        r = oracle.spmv_acc(A, np.zeros_like(zg2[0]), zg2[0]) - eg2[0] * zg2[0]
        assert np.linalg.norm(r) < 1e-5
    # the same matrix handed over as a CSR (the reference's route, DefaultSymmetry.h:54-57): block detected, T / C / D read off it, every row verified
    with LanczosEngine(dtype="c128") as e, LanczosEngine(dtype="c128") as d:
        e.set_csr(A.rowptr, A.colind, A.values)
        d.assemble_hubbard(L, nup, ndown, hop, U, V)
        assert e.layout()["kernel"] == 4 and e.layout() == d.layout()
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind)
        assert np.array_equal(np.ascontiguousarray(va).view(np.uint64), np.ascontiguousarray(A.values).view(np.uint64))
        assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL
        if case == "peierls_ring":  # one changed value: not a product-basis matrix any more
            B = oracle.Csr(A.rowptr.copy(), A.colind.copy(), A.values.copy())
            r = A.nrows // 2 + 17
            k = A.rowptr[r] + (0 if A.colind[A.rowptr[r]] != r else 1)
            B.values[k] *= 1.5
            e.set_csr(B.rowptr, B.colind, B.values)
            assert e.layout()["kernel"] != 4
            assert rel(e.matrixVectorProduct(x0.copy(), y), oracle.spmv_acc(B, x0.copy(), y)) < SPMV_TOL
    monkeypatch.setenv("LPP_PB_COMPLEX", "0")  # the general layout gives the same numbers
    with LanczosEngine(dtype="c128") as e:
        e.assemble_hubbard(L, nup, ndown, hop, U, V)
        assert e.layout()["kernel"] != 4
        assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL


@pytest.mark.parametrize("case,form", [("peierls_ring", "pieces"), ("kane_mele_like", "pieces"), ("disorder", "pieces"), ("peierls_ring", "pieces_wide"),
                                       ("peierls_ring", "pieces_one_block")])
def test_complex_hoppings_beyond_one_lds_window(case, form, monkeypatch):
    """Complex hoppings with rows that do not fit one LDS window (4x4 lattice at 7/8 up electrons: 12870 complex positions): the realified
    in-block matrix is cut into pieces like any real one (four value groups: two blocks per workgroup since round 5, k_pb_up_big2<.., 4, 2>;
    `pieces_one_block`: k_pb_up_big<.., 4, 3>), the couplings stay complex (k_pb_down<CPLX>, with 64-bit addresses for vectors beyond 4 GiB).
    Small case, pieces of 256 positions forced; same checks as the one-window test."""
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")
    monkeypatch.setenv("LPP_PB_PIECE_ROWS", "256")
    if form == "pieces_wide":
        monkeypatch.setenv("LPP_PB_WIDE", "1")
    if form == "pieces_one_block":
        monkeypatch.setenv("LPP_PB_BIG2_FOUR", "0")
    L, nup, ndown = 12, 6, 5
    ring = chain(L, -1.0, True).astype(complex)
    up = np.triu(np.ones((L, L)), 1) > 0
    if case == "kane_mele_like":
        nnn = (np.diag(np.ones(L - 2), 2) + np.diag(np.ones(L - 2), -2)).astype(complex)
        hop = ring + 0.3j * np.where(up, nnn, -nnn)
    else:
        hop = ring * np.where(up, np.exp(0.37j), np.exp(-0.37j))
    U = np.full(L, 4.0) if case != "disorder" else np.random.default_rng(5).uniform(1, 5, L)
    V = np.zeros(2 * L) if case != "disorder" else np.random.default_rng(6).uniform(-0.5, 0.5, 2 * L)
    A = oracle.hubbard_csr(L, nup, ndown, hop, U, V)
    x0, y = oracle.fill_random(A.nrows, 7, True), oracle.fill_random(A.nrows, 8, True)
    xo = oracle.spmv_acc(A, x0.copy(), y)
    init = oracle.fill_random(A.nrows, 4321, True)
    eo, zo, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234, True), nstates=1)
    steps_o, ao, bo, _, _ = oracle.lanczos_decomposition(A, init)
    with LanczosEngine(dtype="c128") as e:
        e.assemble_hubbard(L, nup, ndown, hop, U, V)
        lay = e.layout()
        assert lay["kernel"] == 4 and lay["nnz"] == A.nnz and lay["pieces"] == 8 and lay["chained_step"] == 0 and lay["segments"] == 0
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind)
        assert np.array_equal(np.ascontiguousarray(va).view(np.uint64), np.ascontiguousarray(A.values).view(np.uint64))
        xg = e.matrixVectorProduct(x0.copy(), y)
        assert rel(xg, xo) < SPMV_TOL
        eg, zg, st = e.lanczos(1, want_vectors=True)
        assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0]) and st["steps"] == so
        r = oracle.spmv_acc(A, np.zeros_like(zg[0]), zg[0]) - eg[0] * zg[0]
        assert np.linalg.norm(r) < 1e-5 and abs(np.linalg.norm(zg[0]) - 1) < 1e-8
        ag, bg, _ = e.decomposition(init)
        assert len(ag) == steps_o and rel(ag, ao) < 1e-8 and rel(bg, bo) < 1e-8
    with LanczosEngine(dtype="c128", save_vectors=0) as e:  # scale-free recurrence + two-pass Ritz vector
        e.assemble_hubbard(L, nup, ndown, hop, U, V)
        eg2, zg2, st2 = e.lanczos(1, want_vectors=True)
        assert st2["vectors_saved"] == 0 and abs(eg2[0] - eo[0]) <= E_TOL * abs(eo[0])
        r = oracle.spmv_acc(A, np.zeros_like(zg2[0]), zg2[0]) - eg2[0] * zg2[0]
        assert np.linalg.norm(r) < 1e-5
    with LanczosEngine(dtype="c128") as e:  # the same matrix handed over as a CSR
        e.set_csr(A.rowptr, A.colind, A.values)
        assert e.layout()["kernel"] == 4 and e.layout()["pieces"] == 8
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind)
        assert np.array_equal(np.ascontiguousarray(va).view(np.uint64), np.ascontiguousarray(A.values).view(np.uint64))
        assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL


def test_product_basis_layout_falls_back_when_it_does_not_apply(monkeypatch):
    """more than 8 distinct in-block values, or a many-valued diagonal with the plain stream switched off (LPP_PB_PLAIN_DIAG=0): the
    general layout takes over, results unchanged"""
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")
    L, nup, ndown = 12, 6, 6
    rng = np.random.default_rng(5)
    for k, (hop, U) in enumerate(((chain(L, -1.0, True), rng.uniform(1, 5, L)),  # random U: 2^12 distinct diagonals
                                  (chain(L, -1.0, True) * np.triu(1 + 0.01 * np.arange(L * L).reshape(L, L), 1) + (chain(L, -1.0, True) * np.triu(1 + 0.01 * np.arange(L * L).reshape(L, L), 1)).T, np.full(L, 4.0)))):
        if k == 0:
            monkeypatch.setenv("LPP_PB_PLAIN_DIAG", "0")
        else:
            monkeypatch.delenv("LPP_PB_PLAIN_DIAG")
        A = oracle.hubbard_csr(L, nup, ndown, hop, U)
        with LanczosEngine() as e:
            e.assemble_hubbard(L, nup, ndown, hop, U)
            assert e.layout()["kernel"] != 4
            y = oracle.fill_random(A.nrows, 8)
            assert rel(e.matrixVectorProduct(np.zeros(A.nrows), y), oracle.spmv_acc(A, np.zeros(A.nrows), y)) < SPMV_TOL


@pytest.mark.parametrize("case", ["small_general", "product_layout"])
def test_hubbard_extended_coulomb_term(case, monkeypatch):
    """Model=HubbardOneBandExtended (ModelSelector.h:76-80): the Coulomb term 0.5 sum_ij V_ij n_i n_j of HubbardHelper.h:167-177 on
    the device assembler (general layout and product-basis layout), bit-exact against the oracle's ninj path, and in the
    matrix-free engine (the term split by species)."""
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")  # where it applies (N_up >= 512): the second case
    if case == "small_general":
        L, nup, ndown = 8, 4, 3
        hop, ninj = square(2, 4, -1.0, False), square(2, 4, 0.75, False) + 0.25 * chain(8, 1.0, True)
        U, V = np.linspace(1.0, 4.5, L), np.linspace(-0.5, 0.5, 2 * L)
    else:
        L, nup, ndown = 12, 6, 5
        hop, ninj = chain(L, -1.0, True), chain(L, 0.5, True)
        U, V = np.full(L, 4.0), np.zeros(2 * L)
    A = oracle.hubbard_csr(L, nup, ndown, hop, U, V, ninj=ninj)
    A0 = oracle.hubbard_csr(L, nup, ndown, hop, U, V)
    assert not np.array_equal(A.values, A0.values)
    x0, y = oracle.fill_random(A.nrows, 7), oracle.fill_random(A.nrows, 8)
    xo = oracle.spmv_acc(A, x0.copy(), y)
    eo, _, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234), want_vectors=False)
    with LanczosEngine() as e:
        e.assemble_hubbard(L, nup, ndown, hop, U, V, ninj=ninj)
        assert e.layout()["kernel"] == (4 if case == "product_layout" else e.layout()["kernel"])
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind) and np.array_equal(_bits(va), _bits(A.values))
        assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL
        eg, _, st = e.lanczos(1, want_vectors=False)
        assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0]) and st["steps"] == so
        e.setup_hubbard_onthefly(L, nup, ndown, hop, U, V, ninj=ninj)
        assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL
        eg, _, st = e.lanczos(1, want_vectors=False)
        assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0]) and st["steps"] == so


HEIS_SPIN_CASES = [  # (L, twiceS, szPlusConst, periodic, field, anisotropy)
    (8, 2, 8, True, True, True),
    (6, 3, 9, False, True, False),
    (6, 2, 5, False, False, True),
    (10, 2, 10, True, False, False),
    (5, 4, 10, True, True, True),
    (4, 7, 14, False, True, False),
    (9, 1, 4, True, True, True),  # S = 1/2 through the digit basis, with the anisotropy term the S = 1/2 entry point lacks
]


@pytest.mark.parametrize("L,twiceS,m,periodic,with_field,with_aniso", HEIS_SPIN_CASES)
def test_heisenberg_any_spin_device_assembly_and_energy(L, twiceS, m, periodic, with_field, with_aniso):
    """Heisenberg.h:242-307 + BasisHeisenberg.h:28-46 for S > 1/2: structure, values and diagonal bit-exact against the oracle
    (literal restatement: scan of all words, linear-scan index), then the energy."""
    rng = np.random.default_rng(100 * L + twiceS)
    jpm, jzz = chain(L, 1.0, periodic), chain(L, 0.7 + 0.1 * twiceS, periodic)
    jpm[0, 1] = jpm[1, 0] = 1.37  # a bond of its own strength: the value table is per term
    field = rng.uniform(-0.3, 0.3, L) if with_field else None
    aniso = rng.uniform(0.1, 0.4, L) if with_aniso else None
    A = oracle.heis_csr(L, twiceS, m, jpm, jzz, field=field, aniso=aniso, literal_index=(L * twiceS <= 20))
    with LanczosEngine(max_steps=300) as e:
        e.assemble_heisenberg(L, m, jpm, jzz, field, twiceS=twiceS, anisotropy=aniso)
        assert e.rows() == A.nrows
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind)
        assert np.array_equal(va.view(np.uint64), A.values.view(np.uint64))
        eg, _, st = e.lanczos(1, want_vectors=False)
    eo, _, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234), want_vectors=False, max_steps=300)
    # symmetric matrices (S <= 1): the north_star bar.  From S = 3/2 on the reference's matrix is not symmetric (below) and the
    # symmetric Lanczos recurrence applied to it is no longer backward stable -- two summation orders (CPU rows, GPU slices) of
    # the SAME bit-identical matrix agree to ~1e-10..1e-9 there, so the bar for those cases is 1e-7
    assert abs(eg[0] - eo[0]) <= (E_TOL if twiceS <= 2 else 1e-7) * abs(eo[0])
    # The reference forms the S+S- value from the LOWERED site's m alone (Heisenberg.h:296-303: m1 = m2 - 1, both factors): for
    # S = 1/2 and S = 1 that is a constant, from S = 3/2 on the matrix is not symmetric.  Parity means reproducing it; the dense
    # check applies where the matrix is symmetric.
    D = A.to_scipy().toarray() if A.nrows <= 4000 else None
    if D is not None and np.array_equal(D, D.T):
        ed = np.linalg.eigvalsh(D)[0]
        assert abs(eg[0] - ed) <= 1e-9 * abs(ed)
    if twiceS >= 3 and D is not None:
        assert not np.array_equal(D, D.T)


def test_heisenberg_spin_against_the_reference_program_fixture():
    """tests/golden/heis_inf_temp.json: outputs of the reference's own stand-alone program (basis size and the sum over the
    basis of sum_bonds m_i m_j) for S = 1/2, 1 and 3/2 -- the device assembler's row count and the trace of its Jzz-only matrix."""
    import json
    import os
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "heis_inf_temp.json")))
    for c in gold["cases"]:
        L, twiceS, per = c["L"], c["twiceS"], bool(c["periodic"])
        if L == 16:
            continue  # 12870 rows: covered by the S = 1/2 tests
        jzz = chain(L, 1.0, per)
        with LanczosEngine() as e:
            e.assemble_heisenberg(L, twiceS * L // 2, np.zeros((L, L)), jzz, twiceS=twiceS, anisotropy=np.zeros(L))
            assert e.rows() == c["count"], c
            rp, ci, va = e.get_csr()
        assert np.array_equal(ci, np.arange(c["count"]))  # no S+S- term: the matrix is its diagonal
        assert abs(va.sum() - c["sum"]) < 1e-9 * max(1.0, abs(c["sum"])), (c, va.sum())


def test_heisenberg_spin_rejects_what_the_reference_basis_cannot_hold():
    L = 4
    with LanczosEngine() as e:
        with pytest.raises(Exception):
            e.assemble_heisenberg(L, 10, chain(L, 1.0), chain(L, 1.0), twiceS=5)  # 2 bits per site cannot hold m + S = 4, 5
        with pytest.raises(Exception):
            e.assemble_heisenberg(L, 99, chain(L, 1.0), chain(L, 1.0), twiceS=2)  # empty sector


@pytest.mark.parametrize("case", ["ladder_real", "chain_long_range", "complex_hops"])
def test_super_hubbard_extended_and_kane_mele(case):
    """Model=SuperHubbardExtended (HubbardHelper.h:158-165 SzSz on the diagonal, :282-343 spin-flip terms with the sign of the
    electrons in between) and Model=KaneMeleHubbard (hoppings = term 0 + term 1, :63-66) on the device assembler: bit-exact
    against the oracle's restatement (itself checked against an independent Jordan-Wigner ED, tests/test_oracle_pins.py)."""
    rng = np.random.default_rng(17)
    if case == "ladder_real":
        L, nup, ndown = 8, 4, 3
        hop, nj, jc = square(2, 4, -1.0, False), square(2, 4, 0.6, False), square(2, 4, 0.8, False)
        dt = "f64"
    elif case == "chain_long_range":
        L, nup, ndown = 10, 5, 5
        hop, nj = chain(L, -1.0, True), chain(L, 0.5, True)
        jc = chain(L, 0.7, True) + 0.35 * (np.diag(np.ones(L - 3), 3) + np.diag(np.ones(L - 3), -3))  # electrons in between
        jc = jc * (1 + 0.1 * rng.random((L, L)))  # not symmetric: J(i,j) != J(j,i) are added separately
        dt = "f64"
    else:
        L, nup, ndown = 8, 4, 4
        t0 = chain(L, -1.0, True).astype(complex)
        t1 = 0.25j * (np.diag(np.ones(L - 1), 1) - np.diag(np.ones(L - 1), -1))  # Kane-Mele-like second term
        hop, nj, jc = t0 + t1, None, chain(L, 0.5, True)
        dt = "c128"
    U, V = np.linspace(3.0, 4.5, L), np.linspace(-0.2, 0.2, 2 * L)
    A = oracle.hubbard_csr(L, nup, ndown, hop, U, V, ninj=nj, jcoup=jc)
    A0 = oracle.hubbard_csr(L, nup, ndown, hop, U, V, ninj=nj)
    assert A.nnz > A0.nnz  # the spin-flip entries are there
    x0, y = oracle.fill_random(A.nrows, 7, A.is_complex), oracle.fill_random(A.nrows, 8, A.is_complex)
    xo = oracle.spmv_acc(A, x0.copy(), y)
    eo, _, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234, A.is_complex), want_vectors=False)
    with LanczosEngine(dtype=dt) as e:
        e.assemble_hubbard(L, nup, ndown, hop, U, V, ninj=nj, jcoup=jc)
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind)
        assert np.array_equal(np.ascontiguousarray(va).view(np.uint64), np.ascontiguousarray(A.values).view(np.uint64))
        assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL
        eg, _, st = e.lanczos(1, want_vectors=False)
        assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0]) and st["steps"] == so
        # SolverOptions=InternalProductOnTheFly for the same model: the reference's lambda applies setJTermOffDiagonal too
        # (HubbardHelper.h:119-129); nothing is stored, every row re-derives its entries from the term list (k_asm_apply)
        e.setup_hubbard_onthefly(L, nup, ndown, hop, U, V, ninj=nj, jcoup=jc)
        assert e.stats()["nnz"] == A.nnz
        with pytest.raises(LppError):
            e.get_csr()
        assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL
        eg, zg, st = e.lanczos(1, want_vectors=True)
        assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0]) and st["steps"] == so
        r = oracle.spmv_acc(A, np.zeros_like(zg[0]), zg[0]) - eg[0] * zg[0]
        assert np.linalg.norm(r) < 1e-5


def test_recurrence_started_from_an_eigenvector(monkeypatch):
    """Lucky breakdown: the start vector is a converged eigenvector, so a_0 = E0 and b_0 ~ 1e-7 * |a_0|.  The chained product-basis
    step derives b_0^2 from |w|^2 (k_b2_from_w): it must stay finite, clip at zero, and stop where the general layout stops."""
    L, nup, ndown = 12, 6, 5
    hop, U = chain(L, -1.0, True), np.full(L, 4.0)
    runs = {}
    for layout in ("1", "0"):
        monkeypatch.setenv("LPP_PRODUCT_LAYOUT", layout)
        with LanczosEngine(max_steps=300, eps=1e-13) as e:
            e.assemble_hubbard(L, nup, ndown, hop, U)
            assert (e.layout()["kernel"] == 4) == (layout == "1")
            eg, zg, _ = e.lanczos(1, want_vectors=True)
        for sv in (0, 1):
            with LanczosEngine(max_steps=50, save_vectors=sv) as e2:
                e2.assemble_hubbard(L, nup, ndown, hop, U)
                a, b, _ = e2.decomposition(zg[0])
            assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(b >= 0)
            assert abs(a[0] - eg[0]) <= 1e-10 * abs(eg[0]) and b[0] < 1e-5
            runs[(layout, sv)] = len(a)
    assert len(set(runs.values())) == 1, runs


@pytest.mark.parametrize("periodic,field", [(False, False), (True, True)])
def test_heisenberg_chain_as_one_block_of_the_segmented_form(periodic, field, monkeypatch):
    """S = 1/2 Heisenberg chain (Heisenberg.h:80-114, 278-307): S+S- moves an up spin and nothing sits between neighbours, so the
    off-diagonal part is the hopping matrix of the up spins in the basis of BasisHeisenberg.h:38-46 -- ONE block of the product-basis
    form.  Round 4: such a matrix takes the in-block kernel decomposed by the high sites of the basis word (pb_chain, k_pb_up_seg with
    one block per workgroup) + the streaming pass.  Round 5: planned from the couplings alone -- no CSR is assembled; the one
    lpp_engine_get_csr hands out is made by re-running the device assembler, so its bits check the assembler, and the layout itself is
    checked by x += H y, the energies and the coefficients below.  Forced here onto
    16 sites (12870 states, segments of <= 252 positions); BASELINE config 3 (L = 28) takes it by itself.  Checks: CSR bits, x += H y,
    energies, coefficients, Ritz vector, reorthogonalised run; periodic chain = the bond between the two ends (constant sign
    (-1)^(n-1) in the hopping picture), site-dependent field = more diagonal values."""
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")
    monkeypatch.setenv("LPP_PB_PIECE_ROWS", "256")
    L, m = 16, 8
    jpm, jzz = chain(L, 1.0, periodic), chain(L, 0.7, periodic)
    h = np.linspace(-0.3, 0.4, L) if field else None
    A = oracle.heis_csr(L, 1, m, jpm, jzz, h) if field else oracle.heis_csr(L, 1, m, jpm, jzz)
    x0, y = oracle.fill_random(A.nrows, 7), oracle.fill_random(A.nrows, 8)
    xo = oracle.spmv_acc(A, x0.copy(), y)
    init = oracle.fill_random(A.nrows, 4321)
    eo, zo, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234), nstates=1)
    steps_o, ao, bo, _, _ = oracle.lanczos_decomposition(A, init)
    with LanczosEngine() as e:
        e.assemble_heisenberg(L, m, jpm, jzz, h)
        lay = e.layout()
        assert lay["kernel"] == 4 and lay["segments"] == 64 and lay["nnz"] == A.nnz and lay["chained_step"] == 0, lay  # 6 high sites
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind) and np.array_equal(_bits(va), _bits(A.values))
        xg = e.matrixVectorProduct(x0.copy(), y)
        assert rel(xg, xo) < SPMV_TOL
        eg, zg, st = e.lanczos(1, want_vectors=True)
        assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0]) and st["steps"] == so
        r = oracle.spmv_acc(A, np.zeros_like(zg[0]), zg[0]) - eg[0] * zg[0]
        assert np.linalg.norm(r) < 1e-5 and abs(np.linalg.norm(zg[0]) - 1) < 1e-8
        ag, bg, _ = e.decomposition(init)
        assert len(ag) == steps_o and rel(ag, ao) < 1e-8 and rel(bg, bo) < 1e-8
    with LanczosEngine(save_vectors=0) as e:  # scale-free recurrence + two-pass Ritz vector
        e.assemble_heisenberg(L, m, jpm, jzz, h)
        eg2, zg2, st2 = e.lanczos(1, want_vectors=True)
        assert st2["vectors_saved"] == 0 and abs(eg2[0] - eo[0]) <= E_TOL * abs(eo[0])
    e3o, _, s3o = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234), nstates=3, max_steps=150, eps=1e-11, reortho=True)
    with LanczosEngine(reortho=True, max_steps=150, eps=1e-11) as e:
        e.assemble_heisenberg(L, m, jpm, jzz, h)
        e3, z3, st3 = e.lanczos(3, want_vectors=True)
        assert st3["steps"] == s3o and rel(e3, e3o) < 1e-8
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "0")  # the general layout: the same numbers
    with LanczosEngine() as e:
        e.assemble_heisenberg(L, m, jpm, jzz, h)
        assert e.layout()["kernel"] != 4
        assert rel(e.matrixVectorProduct(x0.copy(), y), xg) < SPMV_TOL
    # couplings beyond neighbours are not a chain: the general layout
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")
    j2 = chain(L, 1.0, False) + 0.5 * (np.diag(np.ones(L - 2), 2) + np.diag(np.ones(L - 2), -2))
    with LanczosEngine() as e:
        e.assemble_heisenberg(L, m, j2, jzz)
        assert e.layout()["kernel"] != 4


def test_heisenberg_periodic_chain_L24_chain_layout_against_the_general_layout(monkeypatch):
    """The chain layout at the window size BASELINE config 3 uses (segments of <= 6435 positions, 9 high sites here), periodic: the bond
    between the two ends carries the constant sign (-1)^(n-1) in the hopping picture.  2,704,156 states: x += H y and the solve against the
    general layout of the same device-assembled matrix, and the CSR handed back bit for bit."""
    L, m = 24, 12
    jpm, jzz = chain(L, 1.0, True), chain(L, 1.0, True)
    res = {}
    for lay_env in ("1", "0"):
        monkeypatch.setenv("LPP_PRODUCT_LAYOUT", lay_env)
        with LanczosEngine(max_steps=300, save_vectors=0) as e:
            e.assemble_heisenberg(L, m, jpm, jzz)
            lay = e.layout()
            assert (lay["kernel"] == 4) == (lay_env == "1"), lay
            if lay_env == "1":
                assert lay["segments"] == 512 and lay["pieces"] > 100
            n = e.rows()
            y = oracle.fill_random(n, 8)
            res[lay_env] = (e.matrixVectorProduct(np.zeros(n), y), e.lanczos(1, want_vectors=False), e.get_csr())
    (x1, (e1, _, s1), c1), (x0, (e0, _, s0), c0) = res["1"], res["0"]
    assert rel(x1, x0) < SPMV_TOL
    assert abs(e1[0] - e0[0]) <= E_TOL * abs(e0[0]) and abs(s1["steps"] - s0["steps"]) <= 1
    assert all(np.array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b) for a, b in zip(c1, c0))
    assert -0.4450 < e1[0] / L < -0.4440  # Bethe ansatz: E0 / L = 1/4 - ln 2 - pi^2 / (12 L^2) + ... = -0.44315 - 0.00143 at L = 24


TJ_CASES = {
    # name: (L, nup, ndown, hop, jpm, jzz, w, potentialV, engine dtype)
    # open chain, two holes, real model in a complex engine (BASELINE config 4's shape: SolverOptions=useComplex with real couplings)
    "chain_c128": lambda: (12, 5, 5, chain(12, -1.0), chain(12, 0.4), chain(12, 0.4), chain(12, -0.1), None, "c128"),
    # 3 x 4 torus, three holes, f64 engine: wrap-around bonds rotate long bit ranges, bonds with different J, potentials (up != down)
    "torus_f64": lambda: (12, 5, 4, square(3, 4, -1.0, pbc=True), square(3, 4, 0.4, pbc=True) * (1 + 0.25 * np.triu(np.ones((12, 12)), 3) + 0.25 * np.tril(np.ones((12, 12)), -3)),
                          square(3, 4, 0.3, pbc=True), square(3, 4, -0.1, pbc=True), np.linspace(-0.2, 0.3, 24), "f64"),
    # complex hopping amplitudes (a Peierls phase on every bond of a ring; the reference does NOT conjugate the reverse direction,
    # TjMultiOrb.h:674-692 -- reproduced): one hole, odd number of occupied sites
    "ring_peierls": lambda: (10, 5, 4, chain(10, -1.0, True) * np.exp(0.3j), chain(10, 0.5, True), chain(10, 0.5, True), chain(10, -0.125, True), None, "c128"),
    # no hole at all: the t-J model is the Heisenberg model of the occupied sites (one block, no moves)
    "no_holes": lambda: (12, 6, 6, chain(12, -1.0, True), chain(12, 0.4, True), chain(12, 0.4, True), chain(12, -0.1, True), None, "f64"),
}


@pytest.mark.parametrize("case", sorted(TJ_CASES))
def test_tj_hole_major_form(case, monkeypatch):
    """The one-orbital t-J model without a stored matrix (round 5, lpp_tj_kernels.h): states ordered (hole configuration, spin pattern of
    the occupied sites), every entry re-derived per product from the block's bonds and hole moves.  Forced onto small lattices here
    (BASELINE config 4 takes it by itself).  Against the oracle's restatement of TjMultiOrb::setupHamiltonian in the reference's
    basis order: the CSR lpp_engine_get_csr regenerates (bit for bit), x += H y, the solve (energy, stopping step, Ritz vector in the
    reference's order), the coefficients from a host start vector, the reorthogonalised run; and the general layout gives the same."""
    L, nup, ndown, hop, jpm, jzz, w, pv, dtype = TJ_CASES[case]()
    cplx = dtype == "c128"
    monkeypatch.setenv("LPP_TJ_LAYOUT", "1")
    A = oracle.tj_csr(L, nup, ndown, hop, jpm, jzz, w, pv, force_complex=cplx)
    x0, y = oracle.fill_random(A.nrows, 7, cplx), oracle.fill_random(A.nrows, 8, cplx)
    xo = oracle.spmv_acc(A, x0.copy(), y)
    init = oracle.fill_random(A.nrows, 4321, cplx)
    eo, zo, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234, cplx), nstates=1)
    steps_o, ao, bo, _, _ = oracle.lanczos_decomposition(A, init)
    with LanczosEngine(dtype=dtype) as e:
        e.assemble_tj(L, nup, ndown, hop, jpm, jzz, w, pv)
        lay = e.layout()
        assert lay["kernel"] == 5 and lay["nnz"] == A.nnz and lay["rows_per_block"] == comb(nup + ndown, nup), lay
        assert lay["resident_bytes"] < 0.2 * 12 * A.nnz
        st = e.stats()
        assert (st["nrows"], st["nnz"]) == (A.nrows, A.nnz)
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind) and np.array_equal(_bits(va), _bits(A.values))
        xg = e.matrixVectorProduct(x0.copy(), y)
        assert rel(xg, xo) < SPMV_TOL
        assert rel(e.matrixVectorProduct(xg.copy(), y) - xg, xo - x0) < 1e-12  # accumulate semantics
        # ring_peierls is NOT Hermitian (the reference keeps h unconjugated for the reverse hop): the recurrence is the oracle's all the
        # same, but its Ritz vector is no eigenvector -- compared with the oracle's vector instead of through a residual
        hermitian = case != "ring_peierls"
        eg, zg, st = e.lanczos(1, want_vectors=True)  # built-in start vector == the oracle's stream in the reference's order
        assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0]) and st["steps"] == so
        if hermitian:
            r = oracle.spmv_acc(A, np.zeros_like(zg[0]), zg[0]) - eg[0] * zg[0]
            assert np.linalg.norm(r) < 1e-5 and abs(np.linalg.norm(zg[0]) - 1) < 1e-8
        assert min(rel(zg[0], zo[0]), rel(zg[0], -zo[0])) < 1e-6  # the oracle's vector up to its sign
        ag, bg, _ = e.decomposition(init)
        assert len(ag) == steps_o and rel(ag, ao) < 1e-8 and rel(bg, bo) < 1e-8
        assert e.bench_spmv(1, 2) > 0
    with LanczosEngine(dtype=dtype, save_vectors=0) as e:  # scale-free recurrence + two-pass Ritz vector
        e.assemble_tj(L, nup, ndown, hop, jpm, jzz, w, pv)
        eg2, zg2, st2 = e.lanczos(1, want_vectors=True)
        assert st2["vectors_saved"] == 0 and abs(eg2[0] - eo[0]) <= E_TOL * abs(eo[0])
        assert min(rel(zg2[0], zo[0]), rel(zg2[0], -zo[0])) < 1e-6
    if hermitian:  # (a symmetric recurrence has no excited-state bar on a non-Hermitian matrix)  # (not Hermitian: the reference keeps h unconjugated for the reverse hop; a symmetric recurrence has no excited-state bar there)
        e3o, _, s3o = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234, cplx), nstates=3, max_steps=150, eps=1e-11, reortho=True)
        with LanczosEngine(dtype=dtype, reortho=True, max_steps=150, eps=1e-11) as e:
            e.assemble_tj(L, nup, ndown, hop, jpm, jzz, w, pv)
            e3, z3, st3 = e.lanczos(3, want_vectors=True)
            assert st3["steps"] == s3o and rel(e3, e3o) < 1e-8
    monkeypatch.setenv("LPP_TJ_LAYOUT", "0")  # the general layout: the same numbers
    with LanczosEngine(dtype=dtype) as e:
        e.assemble_tj(L, nup, ndown, hop, jpm, jzz, w, pv)
        assert e.layout()["kernel"] in (1, 2, 3)
        assert rel(e.matrixVectorProduct(x0.copy(), y), xg) < SPMV_TOL


@pytest.mark.parametrize("case", ["chain_c128", "torus_f64"])
def test_tj_csr_handed_over_with_its_model_description(case, monkeypatch):
    """The reference's hand-over (lpp_engine_set_csr of the host-assembled matrix) with lpp_engine_set_model_tj in front of it: the engine
    regenerates the matrix from the description, compares it with the CSR bit for bit and takes the hole-major form -- same layout, products
    and energies as lpp_engine_assemble_tj, and lpp_engine_get_csr returns the uploaded bits.  One changed value in the CSR, or a description
    that is not this matrix, keeps the general layout of the CSR as handed over (and computes with THAT matrix)."""
    L, nup, ndown, hop, jpm, jzz, w, pv, dtype = TJ_CASES[case]()
    cplx = dtype == "c128"
    monkeypatch.setenv("LPP_TJ_LAYOUT", "1")
    A = oracle.tj_csr(L, nup, ndown, hop, jpm, jzz, w, pv, force_complex=cplx)
    x0, y = oracle.fill_random(A.nrows, 7, cplx), oracle.fill_random(A.nrows, 8, cplx)
    xo = oracle.spmv_acc(A, x0.copy(), y)
    eo, _, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234, cplx), nstates=1, want_vectors=False)
    with LanczosEngine(dtype=dtype) as e:
        e.set_model_tj(L, nup, ndown, hop, jpm, jzz, w, pv)
        e.set_csr(A.rowptr, A.colind, A.values)
        lay = e.layout()
        assert lay["kernel"] == 5 and lay["nnz"] == A.nnz, lay
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind) and np.array_equal(_bits(va), _bits(A.values))
        assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL
        eg, _, st = e.lanczos(1, want_vectors=False)
        assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0]) and st["steps"] == so
        # the description is used for ONE matrix: the next plain upload is a plain upload
        e.set_csr(A.rowptr, A.colind, A.values)
        assert e.layout()["kernel"] in (1, 2, 3)
        # a CSR that is not the described model's: one value changed
        vals = A.values.copy()
        k = int(A.rowptr[A.nrows // 2]) + 1
        vals[k] = vals[k] * 1.5 + 0.25
        B = oracle.Csr(A.rowptr, A.colind, vals)
        e.set_model_tj(L, nup, ndown, hop, jpm, jzz, w, pv)
        e.set_csr(B.rowptr, B.colind, B.values)
        assert e.layout()["kernel"] in (1, 2, 3)
        assert rel(e.matrixVectorProduct(x0.copy(), y), oracle.spmv_acc(B, x0.copy(), y)) < SPMV_TOL
        # a description of another model (J doubled) with the right CSR: the CSR wins
        e.set_model_tj(L, nup, ndown, hop, 2 * np.asarray(jpm), jzz, w, pv)
        e.set_csr(A.rowptr, A.colind, A.values)
        assert e.layout()["kernel"] in (1, 2, 3)
        assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL


def test_heisenberg_chain_csr_handed_over_with_its_model_description(monkeypatch):
    """The same for a spin chain: lpp_engine_set_model_heisenberg + lpp_engine_set_csr -> one block of the segmented form (no CSR kept)."""
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")
    monkeypatch.setenv("LPP_PB_PIECE_ROWS", "256")
    L, m = 16, 8
    jpm, jzz, h = chain(L, 1.0, True), chain(L, 0.7, True), np.linspace(-0.3, 0.4, L)
    A = oracle.heis_csr(L, 1, m, jpm, jzz, h)
    x0, y = oracle.fill_random(A.nrows, 7), oracle.fill_random(A.nrows, 8)
    xo = oracle.spmv_acc(A, x0.copy(), y)
    eo, _, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234), nstates=1, want_vectors=False)
    with LanczosEngine() as e:
        e.set_model_heisenberg(L, m, jpm, jzz, h)
        e.set_csr(A.rowptr, A.colind, A.values)
        lay = e.layout()
        assert lay["kernel"] == 4 and lay["segments"] == 64 and lay["nnz"] == A.nnz, lay
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind) and np.array_equal(_bits(va), _bits(A.values))
        assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL
        eg, _, st = e.lanczos(1, want_vectors=False)
        assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0]) and st["steps"] == so
        e.set_model_heisenberg(L, m, jpm, 1.25 * jzz, h)  # not this matrix: the CSR as handed over
        e.set_csr(A.rowptr, A.colind, A.values)
        assert e.layout()["kernel"] != 4
        assert rel(e.matrixVectorProduct(x0.copy(), y), xo) < SPMV_TOL


def _special(k):
    return lambda kernel: kernel == k


def _general(kernel):
    return kernel != 4


def _general_tj(kernel):
    return kernel in (1, 2, 3)


# environment beside the forcing switch -> what layout()["kernel"] must satisfy, per builder.  Read off the code as it stood when the four
# admission gates were still four copies; LPP_KEEP_PLAIN_CSR and "LPP_COMPRESS_VALUES set to anything" are where the copies differ.
GATE_ROWS = [
    #                                hubbard_assembled, csr_uploaded, heisenberg_chain, tj
    ({},                             (_special(4), _special(4), _special(4), _special(5))),
    (dict(LPP_SHARED_OFFSETS="1"),   (_general, _general, _general, _general_tj)),
    (dict(LPP_SPMV_KERNEL="2"),      (_general, _general, _general, _general_tj)),
    (dict(LPP_COMPRESS_VALUES="1"),  (_special(4), _special(4), _special(4), _general_tj)),
    (dict(LPP_COMPRESS_VALUES="0"),  (_general, _general, _general, _general_tj)),
    (dict(LPP_KEEP_PLAIN_CSR="1"),   (_special(4), _special(4), _general, _general_tj)),
]
GATE_BUILDERS = ["hubbard_assembled", "csr_uploaded", "heisenberg_chain", "tj"]


@pytest.mark.parametrize("builder", GATE_BUILDERS)
def test_general_layout_switches_keep_the_special_layouts_out(builder, monkeypatch):
    """Characterisation of the admission gate in front of the four special-layout builders (assemble_hubbard_pb, pb_from_csr, pb_chain,
    tj_build): with its forcing switch set to 1 every builder takes its layout, a switch of the general layout keeps it out, and the
    result is the oracle's x += H y either way.  The rows also pin the differences the gates have inherited (the chain and the t-J form
    list LPP_KEEP_PLAIN_CSR, the t-J form refuses LPP_COMPRESS_VALUES whatever its value); they assert nothing about whether those are right."""
    col = GATE_BUILDERS.index(builder)
    dtype = "f64"
    if builder in ("hubbard_assembled", "csr_uploaded"):
        L, nup, ndown, hop, U, V = PB_CASES["ladder_2x6"]()  # L = 12, (6, 6)
        A = oracle.hubbard_csr(L, nup, ndown, hop, U, V)
        force = dict(LPP_PRODUCT_LAYOUT="1")
        if builder == "hubbard_assembled":
            build = lambda e: e.assemble_hubbard(L, nup, ndown, hop, U, V)
        else:
            build = lambda e: e.set_csr(A.rowptr, A.colind, A.values)
    elif builder == "heisenberg_chain":
        L, m = 16, 8
        jpm, jzz = chain(L, 1.0, False), chain(L, 0.7, False)
        A = oracle.heis_csr(L, 1, m, jpm, jzz)
        force = dict(LPP_PRODUCT_LAYOUT="1", LPP_PB_PIECE_ROWS="256")
        build = lambda e: e.assemble_heisenberg(L, m, jpm, jzz, None)
    else:
        L, nup, ndown, hop, jpm, jzz, w, pv, dtype = TJ_CASES["no_holes"]()  # the smallest: 924 states
        A = oracle.tj_csr(L, nup, ndown, hop, jpm, jzz, w, pv)
        force = dict(LPP_TJ_LAYOUT="1")
        build = lambda e: e.assemble_tj(L, nup, ndown, hop, jpm, jzz, w, pv)
    x0, y = oracle.fill_random(A.nrows, 7), oracle.fill_random(A.nrows, 8)
    xo = oracle.spmv_acc(A, x0.copy(), y)
    for k, v in force.items():
        monkeypatch.setenv(k, v)
    for env, expect in GATE_ROWS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with LanczosEngine(dtype=dtype) as e:
            build(e)
            kernel = e.layout()["kernel"]
            err = rel(e.matrixVectorProduct(x0.copy(), y), xo)
        print(builder, env, "kernel", kernel, "error", err)
        assert expect[col](kernel), (builder, env, kernel)
        assert err < SPMV_TOL, (builder, env, err)
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("source", ["assembled", "uploaded"])
@pytest.mark.parametrize("pitched", [0, 1])
def test_plain_format_window_layout_outs_first_and_pitched(source, pitched, monkeypatch):
    """A matrix in the plain 12-byte format (no value dictionary, no shared offsets: what the `generic_csr` leg of bench.py measures) in the
    window kernel's layout of round 5: a row's entries that leave its row block sit in its first slots (one load per 512-byte run of the
    source vector), and -- pitched = 1, taken by itself from 256 MB per vector on -- the vectors are pitched to 128-byte lines per row block
    (N_up = 924 = 12 mod 16 here), the stored columns being pitched positions.  Both are invisible at the boundary: lpp_engine_get_csr returns
    the CSR bit for bit, vectors cross in the basis order; products, energies, coefficients and Ritz vectors against the oracle."""
    L, nup, ndown = 12, 6, 5
    hop, U, V = chain(L, -1.0, True), np.where(np.arange(L) % 3 == 0, 2.0, 4.0), np.tile([0.25, -0.5, 0.0], 8)
    for k, v in (("LPP_COMPRESS_VALUES", "0"), ("LPP_SHARED_OFFSETS", "0"), ("LPP_PRODUCT_LAYOUT", "0"), ("LPP_LOCAL16", "0"), ("LPP_PITCH_ROWS", str(pitched))):
        monkeypatch.setenv(k, v)
    A = oracle.hubbard_csr(L, nup, ndown, hop, U, V)
    x0, y = oracle.fill_random(A.nrows, 7), oracle.fill_random(A.nrows, 8)
    xo = oracle.spmv_acc(A, x0.copy(), y)
    init = oracle.fill_random(A.nrows, 4321)
    eo, zo, so = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234), nstates=1)
    steps_o, ao, bo, _, _ = oracle.lanczos_decomposition(A, init)
    for save in (-1, 0):
        with LanczosEngine(compress_values=0, save_vectors=save) as e:
            if source == "assembled":
                e.assemble_hubbard(L, nup, ndown, hop, U, V)
            else:
                e.set_row_block(comb(L, nup))
                e.set_csr(A.rowptr, A.colind, A.values)
            lay = e.layout()
            assert lay["kernel"] == 3 and lay["coded"] == 0 and lay["shared_stride"] == 0, lay
            rp, ci, va = e.get_csr()
            assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind) and np.array_equal(_bits(va), _bits(A.values))
            xg = e.matrixVectorProduct(x0.copy(), y)
            assert rel(xg, xo) < SPMV_TOL
            eg, zg, st = e.lanczos(1, want_vectors=True)
            assert abs(eg[0] - eo[0]) <= E_TOL * abs(eo[0]) and st["steps"] == so
            r = oracle.spmv_acc(A, np.zeros_like(zg[0]), zg[0]) - eg[0] * zg[0]
            assert np.linalg.norm(r) < 1e-5 and abs(np.linalg.norm(zg[0]) - 1) < 1e-8
            ag, bg, _ = e.decomposition(init)
            assert len(ag) == steps_o and rel(ag, ao) < 1e-8 and rel(bg, bo) < 1e-8


# The Hubbard chain of test_plain_format_window_layout_outs_first_and_pitched kept in the general layout: 792 row blocks of 924 rows (more
# than twice the CU count: the window kernel is taken without forcing; 924 = 12 mod 16: pitching has something to do).
_PLAIN_FORMAT = dict(LPP_COMPRESS_VALUES="0", LPP_SHARED_OFFSETS="0", LPP_LOCAL16="0")
GENERAL_SWITCH_ROWS = {
    "defaults": {},
    "local16_0": dict(LPP_LOCAL16="0"),
    "diag_codes_0": dict(LPP_DIAG_CODES="0"),
    "block_template_0": dict(LPP_BLOCK_TEMPLATE="0"),
    "template_pack_0": dict(LPP_TEMPLATE_PACK="0"),
    "shared_offsets_0": dict(LPP_SHARED_OFFSETS="0"),
    "compress_values_0": dict(LPP_COMPRESS_VALUES="0"),
    "plain_outs_first_0": dict(_PLAIN_FORMAT, LPP_OUTS_FIRST="0"),
    "plain_pitch_rows_1": dict(_PLAIN_FORMAT, LPP_PITCH_ROWS="1"),
    "spmv_kernel_1": dict(LPP_SPMV_KERNEL="1"),
    "spmv_kernel_2": dict(LPP_SPMV_KERNEL="2"),
    "spmv_kernel_3": dict(LPP_SPMV_KERNEL="3"),
    "window_rows_4096": dict(LPP_WINDOW_ROWS="4096"),
    "spmv_g_32_kernel_1": dict(LPP_SPMV_G="32", LPP_SPMV_KERNEL="1"),
    "keep_plain_csr_1": dict(LPP_KEEP_PLAIN_CSR="1"),
    "detect_block_0": dict(LPP_DETECT_BLOCK="0"),  # on the uploaded matrix without set_row_block
}
_GENERAL_ORACLE = {}


def _general_oracle():
    if not _GENERAL_ORACLE:
        L, nup, ndown = 12, 6, 5
        hop, U, V = chain(L, -1.0, True), np.where(np.arange(L) % 3 == 0, 2.0, 4.0), np.tile([0.25, -0.5, 0.0], 8)
        A = oracle.hubbard_csr(L, nup, ndown, hop, U, V)
        x0, y = oracle.fill_random(A.nrows, 7), oracle.fill_random(A.nrows, 8)
        _GENERAL_ORACLE.update(model=(L, nup, ndown, hop, U, V), A=A, x0=x0, y=y, xo=oracle.spmv_acc(A, x0.copy(), y))
        for a in (A.rowptr, A.colind, A.values, x0, y, _GENERAL_ORACLE["xo"]):
            a.setflags(write=False)
    return _GENERAL_ORACLE


def _general_build(e, source):
    """assembled / uploaded (with set_row_block) / unhinted (uploaded, nobody names the basis block)"""
    O = _general_oracle()
    L, nup, ndown, hop, U, V = O["model"]
    A = O["A"]
    if source == "assembled":
        e.assemble_hubbard(L, nup, ndown, hop, U, V)
    else:
        if source == "uploaded":
            e.set_row_block(comb(L, nup))
        e.set_csr(A.rowptr, A.colind, A.values)


def _general_sources(row):
    return ("unhinted",) if row == "detect_block_0" else ("assembled", "uploaded")


# layout() of every row above, recorded from a run of this test at the commit BEFORE the general layout's build moved into lpp_csr_plan.h /
# lpp_csr_layout.hip; both sources of a row gave the same dictionary.  Written as the fields that differ from the defaults' row.
_GENERAL_DEFAULTS = dict(kernel=3, coded=1, local16=1, shared_stride=16, block_template=2, diagonal_codes=1, nnz=10178784, per_row_entries=4283136,
                         shared_entries=83520, rows_per_block=924, resident_bytes=14751456, stream_bytes=3042512, pieces=0, coupling_parts=0,
                         diagonal_plain=0, chained_step=0, split_panel=0, rows_by_list_length=0, segments=0, coupling_rounds=0)
_GENERAL_PLAIN = dict(coded=0, local16=0, shared_stride=0, block_template=0, diagonal_codes=0, per_row_entries=10178784, shared_entries=0)
_GENERAL_ONE_BLOCK = dict(kernel=2, local16=0, block_template=0, diagonal_codes=0, per_row_entries=5064992, shared_entries=79904, rows_per_block=731808,
                          resident_bytes=48828176, stream_bytes=37119232)
GENERAL_LAYOUTS = {
    "defaults": dict(),
    "local16_0": dict(local16=0, block_template=0, resident_bytes=45111488, stream_bytes=33402544),
    "diag_codes_0": dict(block_template=1, diagonal_codes=0, per_row_entries=5014944, resident_bytes=25863232, stream_bytes=14154288),
    "block_template_0": dict(block_template=0, resident_bytes=36545088, stream_bytes=24836144),
    "template_pack_0": dict(),  # the packed copy is counted in neither byte figure: only the product shows it
    "shared_offsets_0": dict(local16=0, shared_stride=0, block_template=0, diagonal_codes=0, per_row_entries=10178784, shared_entries=0,
                             resident_bytes=66026136, stream_bytes=60171664),
    "compress_values_0": dict(coded=0, block_template=0, diagonal_codes=0, per_row_entries=5014944, resident_bytes=67162264, stream_bytes=55453320),
    "plain_outs_first_0": dict(_GENERAL_PLAIN, resident_bytes=131022928, stream_bytes=125168456),  # the order inside a row and the pitch are
    "plain_pitch_rows_1": dict(_GENERAL_PLAIN, resident_bytes=131022928, stream_bytes=125168456),  # invisible here: get_csr and the product
    "spmv_kernel_1": dict(_GENERAL_PLAIN, kernel=1, rows_per_block=0, resident_bytes=127999880, stream_bytes=127999880),
    "spmv_kernel_2": _GENERAL_ONE_BLOCK,
    "spmv_kernel_3": dict(),
    "window_rows_4096": dict(local16=0, block_template=0, per_row_entries=4333184, shared_entries=79904, rows_per_block=4096, resident_bytes=45089344,
                             stream_bytes=33380400),
    "spmv_g_32_kernel_1": dict(_GENERAL_PLAIN, kernel=1, rows_per_block=0, resident_bytes=127999880, stream_bytes=127999880),
    "keep_plain_csr_1": dict(resident_bytes=136896864),
    "detect_block_0": _GENERAL_ONE_BLOCK,  # no block: the locality count of a 16384-row window stays below 0.35, one block of all rows
}


def _general_expected(row):
    return dict(_GENERAL_DEFAULTS, **GENERAL_LAYOUTS[row])


def _general_check(e, row, source):
    O = _general_oracle()
    A = O["A"]
    lay = e.layout()
    print(row, source, lay)
    assert lay == _general_expected(row), (row, source, lay)
    rp, ci, va = e.get_csr()
    assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind) and np.array_equal(_bits(va), _bits(A.values)), (row, source)
    err = rel(e.matrixVectorProduct(O["x0"].copy(), O["y"]), O["xo"])
    print(row, source, "error", err)
    assert err < SPMV_TOL, (row, source, err)
    return lay


@pytest.mark.parametrize("row", list(GENERAL_SWITCH_ROWS) + ["per_build_pair"])
def test_general_layout_switches_select_their_forms(row, monkeypatch):
    """Characterisation of the general CSR layout's build (finalize_csr and what it calls): under every switch the build reads, the matrix
    gets exactly the layout the table records -- the whole layout() dictionary, byte figures included, which is all that shows
    LPP_TEMPLATE_PACK -- lpp_engine_get_csr returns the oracle's CSR bit for bit and x += H y is the oracle's.  The last case builds two
    engines in one process with a switch changed between them: the switches are read at every build, never once per process."""
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "0")
    if row == "per_build_pair":
        monkeypatch.setenv("LPP_LOCAL16", "0")
        with LanczosEngine() as first:
            _general_build(first, "uploaded")
            monkeypatch.delenv("LPP_LOCAL16")
            with LanczosEngine() as second:
                _general_build(second, "uploaded")
                l1 = _general_check(first, "local16_0", "uploaded")
                l2 = _general_check(second, "defaults", "uploaded")
        assert l1 != l2 and (l1["local16"], l2["local16"]) == (0, 1)
        return
    for k, v in GENERAL_SWITCH_ROWS[row].items():
        monkeypatch.setenv(k, v)
    for source in _general_sources(row):
        with LanczosEngine() as e:
            _general_build(e, source)
            _general_check(e, row, source)
