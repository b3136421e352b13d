"""No GPU: keeps the long-double reference of tests/lanczos_reference.py and the inputs of tests/test_gpu_lanczos_steps.py honest.

The reference against the C oracle and against dense diagonalisation; then, for every case and seed the GPU tests use, the two input conditions that
make a per-step bound of a few eps meaningful: no compared b_j below 0.05 |H|_inf, and no twin further than 8 eps |H|_inf from the reference (so
that 8 |twin - reference| never exceeds 64 eps |H|_inf)."""
import numpy as np
import pytest

import lanczos_reference as R
import oracle
from helpers import rel

EPS = R.EPS


def _conditions(H, init, K, forms, reortho=False, vectors=False):
    """the input conditions of one case for the given twin forms; returns the largest |twin - reference| / (eps |H|_inf) per form"""
    hn = R.norm_inf(H)
    ar, br, Vr = R.reference(H, init, K, reortho)
    steps = len(ar)
    assert steps == min(K, H.n)
    nb = R.compared(steps, H.n)
    if nb:
        assert float(br[:nb].min()) >= R.B_FLOOR * hn, "b_%d = %.3g |H|_inf" % (int(np.argmin(br[:nb])), float(br[:nb].min()) / hn)
    if steps == H.n:  # the b of the exhausting step is rounding noise, never compared
        assert float(br[-1]) <= 1e-10 * max(1.0, hn)
    worst = {}
    for f in forms:
        at, bt, Vt = R.twin(H, init, K, f)
        assert len(at) == steps
        d = max(float(np.abs(at - ar).max()), float(np.abs(bt[:nb] - br[:nb]).max()) if nb else 0.0)
        assert R.FACTOR * d <= R.COND_FACTOR * EPS * hn, (f, d / (EPS * max(hn, 1e-300)))
        if steps == H.n and f != "derived_norm":  # (the derived norm leaves sqrt(eps) |H| there: a difference of squares; no exhausting run takes it)
            assert bt[-1] <= 1e-10 * max(1.0, hn)
        worst[f] = d / (EPS * hn) if hn > 0 else 0.0
        if vectors:  # cases whose Lanczos vectors are compared: still well conditioned at step K, directly and through the Ritz-vector route
            assert R.vector_deviation(Vt, Vr).max() <= R.VECTOR_COND * EPS, f
            assert R.vector_deviation(R.ritz_route(at, bt, Vt, R.numpy_eigh), Vr).max() <= R.VECTOR_COND * EPS, f
    return worst


@pytest.mark.parametrize("cplx", [False, True])
def test_reference_agrees_with_the_oracle(cplx):
    case = R.case_a(513 if cplx else 257, cplx)
    H, init = R.build(case), R.init_of(case)
    A = oracle.Csr(H.rowptr, H.colind, H.values)
    for reortho in (False, True):
        steps, ao, bo, _, _ = oracle.lanczos_decomposition(A, init, max_steps=case.K, eps=0.0, reortho=reortho)
        ar, br, Vr = R.reference(H, init, case.K, reortho)
        assert steps == len(ar) == case.K
        assert rel(ao, ar.astype(np.float64)) < 1e-10 and rel(bo, br.astype(np.float64)) < 1e-10
        assert ar.dtype == np.longdouble and Vr[0].dtype == (np.clongdouble if cplx else np.longdouble)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 9])
def test_reference_tridiagonal_matrix_has_the_spectrum_of_the_dense_one(n, cplx):
    """K = n steps exhaust the space: T is unitarily similar to H"""
    seed = R.SEEDS_A.get((n, cplx), 3)
    H, init = R.hermitian_csr(n, cplx, seed), R.start_vector(n, cplx, seed + 1000)
    A = R.dense(H)
    assert np.array_equal(A, A.conj().T)
    for reortho in (False, True):
        a, b, V = R.reference(H, init, n, reortho)
        assert len(a) == n
        T = np.diag(a.astype(np.float64)) + np.diag(b.astype(np.float64)[:n - 1], 1) + np.diag(b.astype(np.float64)[:n - 1], -1)
        w = np.linalg.eigvalsh(A)
        assert np.abs(np.linalg.eigvalsh(T) - w).max() <= 1e-13 * max(1.0, np.abs(w).max())
        assert float(b[-1]) <= 1e-10 * max(1.0, R.norm_inf(H))  # rounding noise in every precision


def test_matrix_builders_and_product():
    for cplx in (False, True):
        H = R.hermitian_csr(257, cplx, 1)
        assert H.rowptr.dtype == np.int64 and H.colind.dtype == np.int32 and H.values.dtype == (np.complex128 if cplx else np.float64)
        per_row = np.diff(H.rowptr)
        assert 6.0 < per_row.mean() < 7.1 and all(np.all(np.diff(H.colind[s:e]) > 0) for s, e in zip(H.rowptr[:-1], H.rowptr[1:]))
        y = R.start_vector(257, cplx, 5)
        assert np.abs(R.product(H, H.values, y) - R.dense(H) @ y).max() < 1e-14
        T = R.tridiagonal_csr(11, cplx, 3)
        assert np.array_equal(R.dense(T), R.dense(T).conj().T) and R.nnz_max(T) == 3
    # empty rows are zero, in any dtype
    E = R.Csr(np.array([0, 0, 2, 2, 3], np.int64), np.array([0, 3, 2], np.int32), np.array([1.0, 2.0, 3.0]), 4)
    for t in (np.float64, np.longdouble, np.clongdouble):
        out = R.product(E, E.values.astype(t), np.array([1.0, 1.0, 2.0, 4.0]).astype(t))
        assert out.dtype == t and np.array_equal(out.real.astype(np.float64), [0.0, 9.0, 0.0, 6.0])
    D = R.diagonal_csr(7, 1)
    assert np.array_equal(R.dense(D), np.diag(D.values)) and R.nnz_max(D) == 1


@pytest.mark.parametrize("case", R.CASES_A + R.CASES_A_K9, ids=lambda c: c.name)
def test_input_conditions_general_layout(case):
    H, init = R.build(case), R.init_of(case)
    vectors = case in R.CASES_B
    _conditions(H, init, case.K, ("normalised", "scalefree", "derived_norm"), vectors=vectors)
    _conditions(H, init, case.K, ("reortho",), reortho=True, vectors=vectors)


@pytest.mark.parametrize("case", R.CASES_C, ids=lambda c: c.name)
def test_input_conditions_grid_stride(case):
    H, init = R.build(case), R.init_of(case)
    assert H.n > (2 if not case.cplx else 1) * 2048 * 256 and (H.n % 2 == 1)  # a second trip of the capped grid; an odd length
    _conditions(H, init, case.K, ("normalised", "scalefree"))
    _conditions(H, init, case.K, ("reortho",), reortho=True)


def test_input_conditions_streamed_pass():
    """the float64 twin is this case's reference: its own distance to long double was measured once (lanczos_reference.CASE_D); here only what
    is cheap at this length: the size is odd, beyond the 256 MiB switch and no multiple of the unrolled stride, and no b_j is small"""
    case = R.CASE_D
    n2 = (case.n + 1) // 2
    blocks = min((n2 + 4 * 256 - 1) // (4 * 256), 16384)  # axpy_blocks
    assert case.n % 2 == 1 and n2 * 32 > (256 << 20) and n2 % (4 * 256) != 0
    assert 3 * blocks * 256 < n2 < 4 * blocks * 256  # most lanes take the unrolled body once, the last ones three trips of the scalar tail loop
    H, init = R.build(case), R.init_of(case)
    a, b, _ = R.twin(H, init, case.K, "normalised")
    assert len(a) == case.K and b.min() >= R.B_FLOOR * R.norm_inf(H)
    assert np.all(R.streamed_bound(H, case.K) <= 64 * EPS * R.norm_inf(H) * (np.arange(case.K) + 1))


@pytest.mark.parametrize("name", ["open_chain_L12", "disorder"])
def test_input_conditions_product_basis(name):
    H = R.pb_matrix(name)
    init = R.start_vector(H.n, False, R.SEED_E)
    _conditions(H, init, R.K_E, R.APPLICABLE["derived_norm" if name == "open_chain_L12" else "scalefree"], vectors=name == "open_chain_L12")


# ---- group F: the cases of tests/test_gpu_pb_down_edges.py ---------------------------------------------------------------------------------
_F = {}


def _f_matrix(name):
    if name not in _F:
        _F[name] = R.pb_matrix(name)
    return _F[name]


@pytest.mark.parametrize("name", list(R.PB_DOWN_CASES))
def test_input_conditions_coupling_kernel_cases(name):
    """every case at its own K, for all three twins (the chained step is held to the derived-norm set, the three-kernel step to a subset of it)"""
    H = _f_matrix(name)
    assert H.n == R.pb_rows(name) and np.iscomplexobj(H.values) == R.pb_is_complex(name)
    K = R.pb_steps(name)
    assert K == (8 if name == "ring_15_2_6" else 16)
    worst = _conditions(H, R.pb_start(name), K, R.APPLICABLE["derived_norm"])
    print("[lanczos-steps] group F %s: largest |twin - reference| / (eps |H|_inf) = %s" % (name, {f: round(v, 3) for f, v in worst.items()}))


# (rows, blocks, blocks per workgroup, shortest and longest coupling list, rowcap) at 256 CUs: 32 coupling workgroups per group
GEOMETRY_256 = {
    "a2a_8_4_1": (560, 8, 1, 7, 7, 8),
    "a2a_8_4_3": (3920, 56, 2, 15, 15, 16),
    "a2a_10_3_5": (30240, 252, 8, 25, 25, 28),
    "a2a_12_2_6": (60984, 924, 29, 36, 36, 36),
    "ttp_ring_11_5_4": (152460, 330, 11, 4, 14, 16),
    "ring_14_2_4": (91091, 1001, 32, 2, 8, 8),
    "ring_15_2_6": (525525, 5005, 157, 2, 12, 12),
    "peierls_11_5_4": (152460, 330, 11, 2, 8, 8),
}


@pytest.mark.parametrize("name", list(R.PB_DOWN_CASES))
def test_geometry_of_the_coupling_kernel_cases(name):
    """what each case is there for, at the 256 CUs of the GPU the suite runs on (tests/test_gpu_pb_down_edges.py asserts the same from the device's count)"""
    from math import comb
    L, nup, ndown, hop = R.pb_case(name)[:4]
    rows, n_blk, ids, lo, hi, rowcap = GEOMETRY_256[name]
    lens = R.coupling_list_lengths(L, ndown, hop)
    assert (R.pb_rows(name), comb(L, ndown), int(lens.min()), int(lens.max())) == (rows, n_blk, lo, hi)
    H = _f_matrix(name)
    assert H.rowptr[-1] == comb(L, nup) * int(lens.sum()) + comb(L, ndown) * int(R.coupling_list_lengths(L, nup, hop).sum()) + rows  # both species' hops and the diagonal
    g = R.down_geometry(n_blk, hi, 256)
    assert (g["grid"], g["slots"], g["ids_per_wg"], g["rowcap"], g["rounds"], g["ids_per_round"]) == (256, 32, ids, rowcap, 1, ids)
    n4 = (hi + 3) // 4  # trip count of the longest list's task: prologue of two chunks, loop unrolled by three
    assert n4 == {"a2a_8_4_1": 2, "a2a_8_4_3": 4, "a2a_10_3_5": 7, "a2a_12_2_6": 9, "ttp_ring_11_5_4": 4, "ring_14_2_4": 2, "ring_15_2_6": 3, "peierls_11_5_4": 2}[name]
    if name == "a2a_8_4_1":
        assert 32 - n_blk == 24 and comb(L, nup) == 70 and (70 + 15) // 16 == 5  # 24 workgroups own nothing; 5 panels for 8 groups
    if name == "a2a_10_3_5":
        assert n_blk == 31 * 8 + 4 and g["rowcap"] == 28 and (28 >> 2) & 1  # full tasks and half a task; the stride is the row capacity itself
    if name == "a2a_12_2_6":
        assert ids == 3 * 8 + 5
        f = R.down_geometry(n_blk, hi, 256, grid=8)  # one workgroup per group owns every block
        assert (f["grid"], f["slots"], f["ids_per_wg"], f["rounds"]) == (8, 1, 924, 1) and (924 + 7) // 8 == 116 and f["lds"] == 140464 and f["lds_pf"] <= 150 * 1024
        f = R.down_geometry(n_blk, hi, 256, grid=8, rounds=2)  # rounds in units of 64
        assert (f["rounds"], f["ids_per_round"]) == (2, 512) and 924 - 512 == 412
        f = R.down_geometry(n_blk, hi, 256, rounds=2)
        assert (f["rounds"], f["ids_per_round"]) == (2, 16)
    if name == "ttp_ring_11_5_4":
        assert (comb(L, nup) + 15) // 16 == 29 and len(np.unique(hop[hop != 0])) == 2  # 29 panels: groups of 4 and of 3; (+-1, +-0.5 with the fermion sign: four values)
    if name == "ring_14_2_4":
        f = R.down_geometry(n_blk, hi, 256, rounds=2)
        assert (f["rounds"], f["ids_per_round"]) == (2, 16) and n_blk - 31 * 32 == 9  # the last workgroup's second round is empty
    if name == "ring_15_2_6":
        assert (ids + 7) // 8 == 20  # tasks against 16 waves
    if name == "peierls_11_5_4":
        assert 2 * comb(L, nup) // 16 >= 8 * 2 + 8  # panels of doubles: enough to wait on


@pytest.mark.parametrize("name", list(R.PB_DOWN_CASES))
def test_elementwise_product_bound_holds_for_the_oracle_and_sees_a_dropped_term(name):
    """the reference alone meets the bound: the C oracle's float64 x0 + H y stays inside product_bound of the long-double product; one term of one
    row left out does not"""
    H = _f_matrix(name)
    cplx = R.pb_is_complex(name)
    x0, y = oracle.fill_random(H.n, 5, cplx), oracle.fill_random(H.n, 6, cplx)
    xr, bound = R.product_reference(H, x0, y), R.product_bound(H, x0, y)
    assert xr.dtype == (np.clongdouble if cplx else np.longdouble) and bound.dtype == np.longdouble and float(bound.min()) > 0.0
    xo = oracle.spmv_acc(oracle.Csr(H.rowptr, H.colind, H.values), x0.copy(), y)
    dev = np.abs(xo.astype(xr.dtype) - xr)
    print("[lanczos-steps] group F %s: oracle product, largest deviation / bound = %.3f" % (name, float((dev / bound).max())))
    assert np.all(dev <= bound)
    i = H.n // 2 + 3
    k = int(H.rowptr[i + 1]) - 1  # the last term of row i
    assert H.values[k] != 0 and y[H.colind[k]] != 0
    xd = xo.copy()
    xd[i] -= H.values[k] * y[H.colind[k]]
    devd = np.abs(xd.astype(xr.dtype) - xr)
    assert devd[i] > bound[i] and np.all(np.delete(devd, i) <= np.delete(bound, i))
