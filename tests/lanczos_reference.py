"""numpy restatement of the three-term recurrence of lpp_lanczos.hip for the per-step tests of the GPU path.

`reference` is the normalised recurrence of that file's header comment in np.longdouble / np.clongdouble; `twin` is the same recurrence in
float64 / complex128 in each of the forms the engine runs (normalised, scale-free, scale-free with the derived norm of k_b2_from_w, blocked
Gram-Schmidt).  The twin shares nothing with the engine: it measures what the algorithm itself costs in double, and `tolerances` turns that into
the bound the device is held to.  Nothing here reads the engine's output.

The cases of tests/test_gpu_lanczos_steps.py are listed here (CASES_A, CASES_B, CASES_C, CASE_D, pb_case) so that tests/test_lanczos_reference_host.py can assert
their input conditions without a GPU.  So are the cases of tests/test_gpu_pb_down_edges.py (PB_DOWN_CASES), with the elementwise bound of a product
(product_bound) and the coupling kernel's launch geometry restated (down_geometry).
"""
from collections import namedtuple

import numpy as np

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
CLD = np.clongdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble is not an extended type on this platform: the reference would be no better than the code under test"

GUARD = 1e-10  # the |b| < 1e-10 guard of LanczosSolver::oneStepDecomposition, as k_swap_scale / epi_coeffs / k_axpy_nrm have it

Csr = namedtuple("Csr", "rowptr colind values n")  # int64 rowptr, int32 colind (what set_csr takes), float64 | complex128 values


# ---- matrices ---------------------------------------------------------------------------------------------------------------------------
def _csr_from_triplets(n, rows, cols, vals, cplx):
    order = np.lexsort((cols, rows))  # rows ascending, columns sorted inside a row
    rows, cols, vals = rows[order], cols[order], vals[order]
    rowptr = np.zeros(n + 1, np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return Csr(np.cumsum(rowptr), cols.astype(np.int32), np.ascontiguousarray(vals, np.complex128 if cplx else np.float64), n)


def hermitian_csr(n, cplx, seed):
    """random sparse Hermitian matrix: about 6 off-diagonal entries per row (3 random pairs per row, mirrored) plus a random diagonal"""
    rng = np.random.default_rng(seed)
    i = rng.integers(0, n, 3 * n)
    j = rng.integers(0, n, 3 * n)
    keep = i != j
    lo, hi = np.minimum(i, j)[keep], np.maximum(i, j)[keep]
    pairs = np.unique(lo.astype(np.int64) * n + hi) if len(lo) else np.zeros(0, np.int64)
    lo, hi = pairs // n, pairs % n
    v = rng.uniform(-1.0, 1.0, len(pairs))
    if cplx:
        v = v + 1j * rng.uniform(-1.0, 1.0, len(pairs))
    d = rng.uniform(-1.0, 1.0, n)
    rows = np.concatenate([lo, hi, np.arange(n)])
    cols = np.concatenate([hi, lo, np.arange(n)])
    vals = np.concatenate([v, np.conj(v), d.astype(v.dtype if cplx else np.float64)])
    return _csr_from_triplets(n, rows, cols, vals, cplx)


def tridiagonal_csr(n, cplx, seed):
    """random diagonal in [-1, 1], off-diagonal moduli in [0.5, 1] (a random phase when complex)"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1.0, 1.0, n)
    o = rng.uniform(0.5, 1.0, max(n - 1, 0))
    if cplx:
        o = o * np.exp(1j * rng.uniform(0.0, 2 * np.pi, max(n - 1, 0)))
    k = np.arange(n - 1)
    rows = np.concatenate([k, k + 1, np.arange(n)])
    cols = np.concatenate([k + 1, k, np.arange(n)])
    vals = np.concatenate([o, np.conj(o), d.astype(o.dtype)])
    return _csr_from_triplets(n, rows, cols, vals, cplx)


def diagonal_csr(n, seed):
    """real diagonal matrix, entries in [-1, 1]"""
    d = np.random.default_rng(seed).uniform(-1.0, 1.0, n)
    return Csr(np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), d, n)


def start_vector(n, cplx, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-0.5, 0.5, n)
    return v + 1j * rng.uniform(-0.5, 0.5, n) if cplx else v


def norm_inf(H):
    """largest absolute row sum"""
    if len(H.values) == 0:
        return 0.0
    rows = np.repeat(np.arange(H.n), np.diff(H.rowptr))
    return float(np.bincount(rows, weights=np.abs(H.values), minlength=H.n).max())


def nnz_max(H):
    return int(np.diff(H.rowptr).max())


def dense(H):
    A = np.zeros((H.n, H.n), H.values.dtype)
    rows = np.repeat(np.arange(H.n), np.diff(H.rowptr))
    np.add.at(A, (rows, H.colind), H.values)
    return A


# ---- the product, in any dtype ------------------------------------------------------------------------------------------------------------
def product(H, va, y):
    """H y with the values given as `va` (H.values in the working dtype): va * y[ci], summed per row; empty rows are zero"""
    out = np.zeros(H.n, np.result_type(va.dtype, y.dtype))
    nonempty = H.rowptr[:-1] < H.rowptr[1:]
    if nonempty.any():
        out[nonempty] = np.add.reduceat(va * y[H.colind], H.rowptr[:-1][nonempty])
    return out


def _dot_re(x, y):
    return np.sum(x.real * y.real + x.imag * y.imag) if np.iscomplexobj(x) else np.sum(x * y)


def _nrm2(x):
    return _dot_re(x, x)


def _gram_schmidt2(V, x):
    """two passes of classical Gram-Schmidt of x against all kept columns"""
    Vm = np.array(V)
    for _ in range(2):
        x = x - Vm.T @ (Vm.conj() @ x)
    return x


def _normalised(H, init, K, real_t, work_t, reortho):
    """lpp_lanczos.hip, header comment: x += H y_j; a_j = Re<y_j|x>; x -= a_j y_j [+ CGS2]; b_j = |x|; (y_{j+1}, x) <- (x/b_j, -b_j y_j)"""
    va = H.values.astype(work_t)
    x0 = np.asarray(init).astype(work_t)
    y = x0 / np.sqrt(_nrm2(x0))
    x = np.zeros(H.n, work_t)
    a, b, V = [], [], []
    for _ in range(min(K, H.n)):
        x = x + product(H, va, y)
        aj = _dot_re(y, x)
        x = x - aj * y
        V.append(y)
        if reortho:
            x = _gram_schmidt2(V, x)
        bj = np.sqrt(_nrm2(x))
        a.append(aj)
        b.append(bj)
        if abs(bj) < GUARD:  # invariant subspace exhausted: the run stops here
            break
        y, x = x / bj, -bj * y
    return np.array(a, real_t), np.array(b, real_t), V


def reference(H, init, K, reortho=False):
    """(a, b, [v_0 .. v_{steps-1}]) in long double"""
    return _normalised(H, init, K, LD, CLD if np.iscomplexobj(H.values) else LD, reortho)


TWIN_FORMS = ("normalised", "scalefree", "derived_norm", "reortho")


def _scalefree(H, init, K, derived):
    """the comment above one_step: r_j = b_{j-1} y_j stays unnormalised; w = H r_j / b_{j-1} - (b_{j-1}/b_{j-2}) r_{j-1}; raw_j = Re<r_j|w> = a_j b_{j-1};
    r_{j+1} = w - (raw_j / b_{j-1}^2) r_j; b_j = |r_{j+1}|.  derived: b_j^2 = |w - s r_j|^2 - (raw_j - s b_{j-1}^2)^2 / b_{j-1}^2 with the shift
    s = a_{j-1} / b_{j-1} of the comment above k_b2_from_w (0 at step 0), the norm of r_{j+1} never being summed."""
    work_t = H.values.dtype
    r = np.asarray(init).astype(work_t)
    rold = np.zeros(H.n, work_t)
    b2 = [float(_nrm2(r))]  # b2[j] = b_{j-1}^2, b_{-1} = |init|
    a, b, V = [], [], []
    s = 0.0
    for j in range(min(K, H.n)):
        b1 = np.sqrt(b2[j])
        alpha = 1.0 if abs(b1) < GUARD else 1.0 / b1
        beta = 0.0
        if j > 0:
            bo = np.sqrt(b2[j - 1])
            beta = -b1 if abs(bo) < GUARD else -b1 / bo
        w = beta * rold + alpha * product(H, H.values, r)
        raw = float(_dot_re(r, w))
        ok = b1 >= GUARD
        g = raw / b2[j] if ok else raw
        rnew = w - g * r
        if derived:
            d = w - s * r
            bj2 = float(_nrm2(d))
            if ok:
                rs = raw - s * b2[j]
                bj2 = bj2 - rs * rs / b2[j]
            bj2 = max(bj2, 0.0)
            s = raw / (b1 * np.sqrt(bj2)) if (ok and np.sqrt(bj2) >= GUARD) else 0.0
        else:
            bj2 = float(_nrm2(rnew))
        a.append(raw / b1 if ok else raw)
        b.append(np.sqrt(bj2))
        V.append(r * alpha)
        b2.append(bj2)
        if b[-1] < GUARD:
            break
        rold, r = r, rnew
    return np.array(a), np.array(b), V


def twin(H, init, K, form):
    """the same recurrence in float64 / complex128, in the form the engine runs it"""
    if form in ("normalised", "reortho"):
        return _normalised(H, init, K, np.float64, H.values.dtype, form == "reortho")
    if form in ("scalefree", "derived_norm"):
        return _scalefree(H, init, K, form == "derived_norm")
    raise ValueError("unknown form %r" % (form,))


# ---- the tolerance rule --------------------------------------------------------------------------------------------------------------------
# The twins whose own deviation from the reference bounds a device form.  A form that is a rearrangement of another (scale-free of normalised,
# derived norm of scale-free) may land on either side of the rearrangement's rounding, so it takes the larger of the two.
APPLICABLE = {
    "normalised": ("normalised",),
    "scalefree": ("normalised", "scalefree"),
    "derived_norm": ("normalised", "scalefree", "derived_norm"),
    "reortho": ("reortho",),
}
FACTOR = 8.0  # another summation order and FMA contraction on the device
COND_FACTOR = 64.0  # input condition: 8 |twin - reference| <= 64 eps |H|_inf, so that no tolerance grows into uselessness
B_FLOOR = 0.05  # input condition: no compared b_j below 0.05 |H|_inf (a near-breakdown step amplifies rounding by |H| / b_j)


def compared(steps, n):
    """how many b_j are compared: the last b of a run that exhausts the space is rounding noise in every precision"""
    return steps - 1 if steps == n else steps


def vector_deviation(Vt, Vr):
    return np.array([float(np.sqrt(_nrm2(np.asarray(t) - r))) for t, r in zip(Vt, Vr)])


def tolerances(H, ref, twins, twin_vectors=None):
    """tol_a[j], tol_b[j] = max(8 max over the twins |twin - reference|, 4 eps |H|_inf), absolute: b may legitimately be tiny;
    tol_v[j] = max(8 |v_j^twin - v_j^ref|_2, 8 eps).  twins: the (a, b, V) of the applicable forms; twin_vectors: the twin's vectors where they went
    through a route of their own (the Ritz-vector route of the vector tests), else those of the last twin listed (the form's own)."""
    ar, br, Vr = ref
    floor = 4.0 * EPS * norm_inf(H)
    steps = len(ar)
    da, db = np.zeros(steps), np.zeros(steps)
    for at, bt, _ in twins:
        assert len(at) == steps
        da = np.maximum(da, np.abs(at.astype(LD) - ar).astype(np.float64))
        db = np.maximum(db, np.abs(bt.astype(LD) - br).astype(np.float64))
    Vt = twins[-1][2] if twin_vectors is None else twin_vectors
    tol_v = np.maximum(FACTOR * vector_deviation(Vt, Vr), FACTOR * EPS)
    return np.maximum(FACTOR * da, floor), np.maximum(FACTOR * db, floor), tol_v


def streamed_bound(H, steps):
    """group D, against the float64 twin: (j+1) (log2 n + nnz_max + 4) eps |H|_inf -- tree summation of n terms plus one row's products"""
    return (np.arange(steps) + 1.0) * (np.log2(H.n) + nnz_max(H) + 4.0) * EPS * norm_inf(H)


def ritz_route(a, b, V, eigh):
    """Z = S^T V as computeAllStatesBelow(nstates = steps) forms it, and back: V' = S Z.  eigh(a, b[:-1]) -> S (steps x steps, orthogonal)"""
    S = eigh(a, b)
    Vm = np.array(V)
    return list(S @ (S.T @ Vm))


def numpy_eigh(a, b):
    k = len(a)
    T = np.diag(np.asarray(a, np.float64)) + np.diag(np.asarray(b, np.float64)[:k - 1], 1) + np.diag(np.asarray(b, np.float64)[:k - 1], -1)
    return np.linalg.eigh(T)[1]


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name kind n cplx seed K")  # kind: hermitian | tridiagonal | diagonal


def build(case):
    if case.kind == "hermitian":
        return hermitian_csr(case.n, case.cplx, case.seed)
    if case.kind == "tridiagonal":
        return tridiagonal_csr(case.n, case.cplx, case.seed)
    return diagonal_csr(case.n, case.seed)


def init_of(case):
    return start_vector(case.n, case.cplx, case.seed + 1000)


SIZES_A = (1, 2, 3, 5, 255, 257, 513, 1025, 2049)
VECTOR_COND = 64.0  # input condition of the cases whose vectors are compared: no twin vector further than 64 eps from the reference's
SEEDS_A = {  # (n, cplx) -> seed; chosen on the CPU so that the input conditions hold (several seeds of the tiny sizes leave a b_j below 0.05 |H|_inf;
    # at 257 real and 513 complex several seeds let a Ritz value start converging within 24 steps, which amplifies the vectors' rounding 300-fold)
    (1, False): 1, (2, False): 1, (3, False): 1, (5, False): 2, (255, False): 1, (257, False): 3, (513, False): 1, (1025, False): 1, (2049, False): 1,
    (1, True): 1, (2, True): 2, (3, True): 1, (5, True): 1, (255, True): 1, (257, True): 1, (513, True): 2, (1025, True): 1, (2049, True): 1,
}
K_A = 24


def case_a(n, cplx, K=K_A):
    return Case("A_%s%d_K%d" % ("c" if cplx else "r", n, min(K, n)), "hermitian", n, cplx, SEEDS_A[(n, cplx)], min(K, n))


CASES_A = [case_a(n, cplx) for cplx in (False, True) for n in SIZES_A]
CASES_A_K9 = [case_a(n, cplx, 9) for cplx in (False, True) for n in SIZES_A if n >= 9]
CASES_B = [case_a(257, False), case_a(2049, False), case_a(513, True)]
CASES_C = [Case("C_r", "tridiagonal", 2 * 2048 * 256 + 3, False, 11, 8), Case("C_c", "tridiagonal", 2048 * 256 + 1, True, 12, 4)]
# group D compares against the float64 normalised twin (long double at this length takes seconds per step).  That twin against long double, measured
# once on the CPU for this input, as a fraction of streamed_bound: a 5.2e-5, 1.3e-4, 8.2e-5; b 0.100, 0.041, 0.001 (steps 0, 1, 2) -- below one eighth
CASE_D = Case("D_r", "diagonal", 16777216 + 2051, False, 13, 3)
# group E: two of PB_CASES of tests/test_gpu_parity.py (restated so that the host test needs no GPU module; the GPU test asserts they are the same)
K_E = 16
SEED_E = 4321


def all_to_all(L, magnitudes, seed):
    """_all_to_all of tests/test_gpu_pb_up_waits.py, restated (that module needs a GPU to import; tests/test_gpu_pb_down_edges.py asserts they agree)"""
    rng = np.random.default_rng(seed)
    m = np.zeros((L, L))
    for i in range(L):
        for j in range(i + 1, L):
            m[i, j] = m[j, i] = rng.choice(magnitudes) * rng.choice([-1.0, 1.0])
    return m


def peierls_ring(L, phase=0.37):
    """_phases of tests/test_gpu_pb_up_staging.py, restated: a ring with a Peierls phase on every bond"""
    from helpers import chain
    up = np.triu(np.ones((L, L)), 1) > 0
    return chain(L, -1.0, True).astype(complex) * np.where(up, np.exp(1j * phase), np.exp(-1j * phase))


# group F (tests/test_gpu_pb_down_edges.py): the coupling kernel's own structure.  name -> (L, n_up, n_down, hopping); U = 4 on every site, no
# potentials.  C(L, n_up) positions per block, C(L, n_down) blocks; a block's coupling list is the down species' hops out of its configuration.
def _ring2(L):
    from helpers import chain
    return chain(L, -1.0, True) + 0.5 * (np.diag(np.ones(L - 2), 2) + np.diag(np.ones(L - 2), -2))


def _ring(L):
    from helpers import chain
    return chain(L, -1.0, True)


PB_DOWN_CASES = {
    "a2a_8_4_1": (8, 4, 1, lambda: all_to_all(8, [1.0], 3)),
    "a2a_8_4_3": (8, 4, 3, lambda: all_to_all(8, [1.0], 3)),
    "a2a_10_3_5": (10, 3, 5, lambda: all_to_all(10, [1.0], 3)),
    "a2a_12_2_6": (12, 2, 6, lambda: all_to_all(12, [1.0], 11)),
    "ttp_ring_11_5_4": (11, 5, 4, lambda: _ring2(11)),
    "ring_14_2_4": (14, 2, 4, lambda: _ring(14)),
    "ring_15_2_6": (15, 2, 6, lambda: _ring(15)),
    "peierls_11_5_4": (11, 5, 4, lambda: peierls_ring(11)),
}
K_F_LARGE_ROWS = 200000  # cases above it run 8 steps, the others 16


def pb_case(name):
    """(L, nup, ndown, hop, U, V)"""
    from helpers import chain
    if name == "open_chain_L12":
        return 12, 6, 6, chain(12, -1.0, False), np.full(12, 4.0), np.zeros(24)
    if name == "disorder":
        return 12, 6, 5, chain(12, -1.0, True), np.random.default_rng(5).uniform(1, 5, 12), np.random.default_rng(6).uniform(-0.5, 0.5, 24)
    if name in PB_DOWN_CASES:
        L, nup, ndown, hop = PB_DOWN_CASES[name]
        return L, nup, ndown, hop(), np.full(L, 4.0), np.zeros(2 * L)
    raise KeyError(name)


def pb_rows(name):
    from math import comb
    L, nup, ndown = (PB_DOWN_CASES[name] if name in PB_DOWN_CASES else pb_case(name))[:3]
    return comb(L, nup) * comb(L, ndown)


def pb_is_complex(name):
    return name == "peierls_11_5_4"


def pb_steps(name):
    return 8 if pb_rows(name) > K_F_LARGE_ROWS else K_E


def pb_matrix(name):
    import oracle
    A = oracle.hubbard_csr(*pb_case(name))
    return Csr(A.rowptr, A.colind, A.values, A.nrows)


def pb_start(name):
    return start_vector(pb_rows(name), pb_is_complex(name), SEED_E)


# ---- the elementwise bound of a product ---------------------------------------------------------------------------------------------------
def product_bound(H, x0, y):
    """bound[i] on |fl(x0 + H y)_i - (x0 + H y)_i| for ANY double-precision evaluation: (nnz_i + 4) 2^-53 (|x0_i| + sum_j |H_ij| |y_j|), the
    first-order forward bound of a sum of nnz_i products accumulated in any order, with or without FMA, plus four more roundings (the scale, the
    diagonal and the two adds of a combine pass).  Complex rows: (2 nnz_i + 6) 2^-53 with moduli (a complex product is two real products and an add
    per component).  Derived, not measured; evaluated in long double."""
    cplx = np.iscomplexobj(H.values) or np.iscomplexobj(y)
    per_row = np.diff(H.rowptr).astype(LD)
    mass = np.abs(np.asarray(x0)).astype(LD) + product(H, np.abs(H.values).astype(LD), np.abs(np.asarray(y)).astype(LD))
    return ((2 * per_row + 6) if cplx else (per_row + 4)) * LD(2.0) ** -53 * mass


def product_reference(H, x0, y):
    """x0 + H y in long double"""
    t = CLD if (np.iscomplexobj(H.values) or np.iscomplexobj(y)) else LD
    return np.asarray(x0).astype(t) + product(H, H.values.astype(t), np.asarray(y).astype(t))


# ---- the coupling kernel's launch geometry, restated -------------------------------------------------------------------------------------------
def coupling_list_lengths(L, ndown, hop):
    """entries of every block's coupling list: hops of the block species (n_down particles) out of each configuration, ascending-word order"""
    from itertools import combinations
    nz = np.asarray(hop) != 0
    np.fill_diagonal(nz, False)
    words = sorted(sum(1 << s for s in occ) for occ in combinations(range(L), ndown))
    out = []
    for w in words:
        occ = [s for s in range(L) if (w >> s) & 1]
        emp = [s for s in range(L) if not (w >> s) & 1]
        out.append(int(sum(nz[i, j] for i in occ for j in emp)))
    return np.array(out)


def _down_lds_bytes(ids, rowcap):
    stride = rowcap if (rowcap >> 2) & 1 else rowcap + 4
    return ((ids * 8 + 15) & ~15) + ids * stride * 4 + 16


def down_geometry(n_blk, longest, num_cus, grid=None, rounds=None):
    """plan_down_geometry / plan_rounds of lpp_pb_plan.cpp for the whole-panel form and vectors below 16 GB: dict(grid, slots, ids_per_wg, rowcap, rounds,
    ids_per_round, lds, lds_pf); 8 CUs at least.  grid: LPP_PB_DOWN_GRID; rounds: LPP_PB_DOWN_ROUNDS"""
    assert num_cus >= 8
    g = num_cus & ~7
    if grid is not None:
        g = max(8, min(grid, g)) & ~7
    slots = g // 8
    rowcap = max(4, (longest + 3) & ~3)
    ids = -(-n_blk // slots)
    unit = 64 if ids >= 512 else 8

    def per_round(r):
        return ids if r == 1 else -(-(-(-ids // r)) // unit) * unit

    r = 1 if rounds is None else max(1, min(rounds, 64))
    while r < 64 and _down_lds_bytes(per_round(r), rowcap) > 150 * 1024:
        r += 1
    while r > 1 and per_round(r) * (r - 1) >= ids:
        r -= 1
    lds = _down_lds_bytes(per_round(r), rowcap)
    return dict(grid=g, slots=slots, ids_per_wg=ids, rowcap=rowcap, rounds=r, ids_per_round=per_round(r), lds=lds, lds_pf=lds + (per_round(r) + 7) // 8 * 32)


_CACHE = {}


def bundle(key, H_fn, init_fn, K, forms, reortho=False, with_reference=True):
    """reference and twins of one case, computed once and shared: dict(H, init, ref, twins={form: (a, b, V)})"""
    if ("in", key) not in _CACHE:
        _CACHE[("in", key)] = (H_fn(), init_fn())
    H, init = _CACHE[("in", key)]
    if with_reference and ("ref", key, K, reortho) not in _CACHE:
        _CACHE[("ref", key, K, reortho)] = reference(H, init, K, reortho)
    for f in forms:
        if ("twin", key, K, f) not in _CACHE:
            _CACHE[("twin", key, K, f)] = twin(H, init, K, f)
    return dict(H=H, init=init, ref=_CACHE.get(("ref", key, K, reortho)), twins={f: _CACHE[("twin", key, K, f)] for f in forms})


def case_bundle(case, form):
    """the bundle of a case of groups A - C for a device form (normalised | scalefree | reortho)"""
    return bundle(case.name, lambda: build(case), lambda: init_of(case), case.K, APPLICABLE[form], reortho=form == "reortho")


def case_tolerances(case, form, twin_vectors=None):
    bd = case_bundle(case, form)
    return bd, tolerances(bd["H"], bd["ref"], [bd["twins"][f] for f in APPLICABLE[form]], twin_vectors)
