"""-m gpu: the first K steps of the device recurrence, step by step, against the long-double reference of tests/lanczos_reference.py.

Before any Ritz value converges the recurrence is well conditioned, so a_j, b_j and the Lanczos vectors are held to a few tens of eps |H|_inf per
step instead of the 1e-8 a converged run allows -- at the lengths and forms no whole solve of the suite reaches: odd real lengths (the padding
double of the last double2), a second trip of the capped BLAS grid, the streamed unrolled body of k_axpy_nrm, Gram-Schmidt panels with a tail, the
in-place swap, the derived norm of the chained step.  The tolerance rule is lanczos_reference.tolerances; nothing in it comes from the engine, and
tests/test_lanczos_reference_host.py asserts the input conditions of every case here.  All runs: eps = 0, max_steps = K, so exactly min(K, n) steps.
Every case prints its largest deviation / tolerance ratio (pytest -s or -rP shows them; DESIGN.md section 3 records them per group)."""
import numpy as np
import pytest
import torch  # loaded before the engine library, so that both use one HIP runtime -- INTEGRATION.md

import lanczos_reference as R
from lanczosplusplus_amd import LanczosEngine, tridiag_lowest

pytestmark = pytest.mark.gpu

LD = np.longdouble
# device form -> (constructor arguments, LPP_NO_SCALE_FREE, the twin form that bounds it)
FORMS = {
    "scalefree": (dict(save_vectors=0), False, "scalefree"),  # k_axpy_nrm<true> with b2_prev, the EpiScale epilogue, no swap pass
    "saved": (dict(save_vectors=1), False, "normalised"),  # k_scale_copy, k_swap_scale writing y_{j+1} into V
    "inplace": (dict(save_vectors=0), True, "normalised"),  # k_swap_scale with y aliasing ynext
    "reortho": (dict(reortho=True), False, "reortho"),  # k_multi_dot / k_multi_axpy panels, k_dot
}


def _report(group, tag, ratio):
    print("[lanczos-steps] group %s %s: largest deviation / tolerance = %.3f" % (group, tag, ratio))


def _dtype(H):
    return "c128" if np.iscomplexobj(H.values) else "f64"


def _engine(H, K, form, monkeypatch, **kw):
    args, no_scale_free, _ = FORMS[form]
    if no_scale_free:
        monkeypatch.setenv("LPP_NO_SCALE_FREE", "1")
    else:
        monkeypatch.delenv("LPP_NO_SCALE_FREE", raising=False)
    e = LanczosEngine(dtype=_dtype(H), max_steps=K, eps=0.0, **args, **kw)
    e.set_csr(H.rowptr, H.colind, H.values)
    return e


def _check_coeffs(group, tag, H, ag, bg, ar, br, tol_a, tol_b):
    steps = len(ar)
    assert len(ag) == len(bg) == steps
    nb = R.compared(steps, H.n)
    da = np.abs(ag.astype(LD) - ar).astype(np.float64)
    db = np.abs(bg.astype(LD) - br).astype(np.float64)[:nb]
    ratio = max(float((da / tol_a).max()), float((db / tol_b[:nb]).max()) if nb else 0.0)
    _report(group, tag, ratio)
    assert np.all(da <= tol_a), (tag, "a", da / tol_a)
    assert np.all(db <= tol_b[:nb]), (tag, "b", db / tol_b[:nb])
    if steps == H.n:  # the exhausting step
        assert bg[-1] <= 1e-10 * max(1.0, R.norm_inf(H)), (tag, bg[-1])
    return ratio


def _run_decomposition(group, case, form, monkeypatch, tag="", **kw):
    bd, (tol_a, tol_b, _) = R.case_tolerances(case, FORMS[form][2])
    H, init = bd["H"], bd["init"]
    with _engine(H, case.K, form, monkeypatch, **kw) as e:
        ag, bg, st = e.decomposition(init)
        assert st["vectors_saved"] == (1 if form in ("saved", "reortho") else 0)
    ar, br, _ = bd["ref"]
    return _check_coeffs(group, "%s %s%s" % (case.name, form, tag), H, ag, bg, ar, br, tol_a, tol_b)


# ---- A: general layout through set_csr ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", R.CASES_A, ids=lambda c: c.name)
def test_coefficients_general_layout(case, form, monkeypatch):
    _run_decomposition("A", case, form, monkeypatch)


@pytest.mark.parametrize("case", R.CASES_A_K9, ids=lambda c: c.name)
def test_reortho_with_a_one_column_tail_panel(case, monkeypatch):
    """K = 9: the ninth column is a panel of its own (kPanel = 8)"""
    _run_decomposition("A", case, "reortho", monkeypatch)


@pytest.mark.parametrize("kernel", [0, 1, 2, 3])
@pytest.mark.parametrize("case", [R.case_a(257, False), R.case_a(513, True)], ids=lambda c: c.name)
def test_scale_free_epilogue_of_every_product_kernel(case, kernel, monkeypatch):
    _run_decomposition("A", case, "scalefree", monkeypatch, tag=" spmv_kernel=%d" % kernel, spmv_kernel=kernel)


@pytest.mark.parametrize("form", ["scalefree", "saved", "inplace", "reortho"])
@pytest.mark.parametrize("case", [R.case_a(257, False), R.case_a(2049, False), R.case_a(513, True)], ids=lambda c: c.name)
def test_incremental_interface_in_uneven_pieces(case, form, monkeypatch):
    bd, (tol_a, tol_b, _) = R.case_tolerances(case, FORMS[form][2])
    H, init = bd["H"], bd["init"]
    ar, br, _ = bd["ref"]
    with _engine(H, case.K, form, monkeypatch) as e:
        e.begin(init)
        done = 0
        for piece in (1, 7, 16):
            e.step(piece)
            done += piece
            e.sync()
            ag, bg = e.coeffs()
            assert len(ag) == done
            da = np.abs(ag.astype(LD) - ar[:done]).astype(np.float64)
            db = np.abs(bg.astype(LD) - br[:done]).astype(np.float64)
            assert np.all(da <= tol_a[:done]) and np.all(db <= tol_b[:done]), (done, da / tol_a[:done], db / tol_b[:done])
        assert done == case.K
    _check_coeffs("A", "%s %s begin/step 1+7+16" % (case.name, form), H, ag, bg, ar, br, tol_a, tol_b)


@pytest.mark.parametrize("form", ["scalefree", "saved"])
@pytest.mark.parametrize("case", [R.case_a(257, False), R.case_a(2049, False)], ids=lambda c: c.name)
def test_device_start_vector_aligned_to_8_bytes_only(case, form, monkeypatch):
    """odd n, the start vector a tensor view that begins 8 bytes into its allocation"""
    bd, (tol_a, tol_b, _) = R.case_tolerances(case, FORMS[form][2])
    H, init = bd["H"], bd["init"]
    buf = torch.zeros(H.n + 1, dtype=torch.float64, device="cuda")
    view = buf[1:]
    view.copy_(torch.from_numpy(init))
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8 and H.n % 2 == 1
    with _engine(H, case.K, form, monkeypatch) as e:
        ag, bg, _ = e.decomposition(init_device=view.data_ptr())
    ar, br, _ = bd["ref"]
    _check_coeffs("A", "%s %s init_device+8" % (case.name, form), H, ag, bg, ar, br, tol_a, tol_b)
    assert np.array_equal(view.cpu().numpy(), init)  # the caller's vector is left alone


# ---- B: the Lanczos vectors themselves ---------------------------------------------------------------------------------------------------------
def _engine_vectors(e, init, K):
    """V = S Z: computeAllStatesBelow(nstates = K) returns Z = S^T V, S the eigenvectors of the engine's own T (lpp_tridiag_lowest, the routine the
    solve called, on the coefficients of that run)"""
    _, zg, st = e.lanczos(K, init=init, want_vectors=True)
    assert st["steps"] == K
    ag, bg = e.coeffs()
    _, S = tridiag_lowest(ag, bg[:-1], K, vectors=True)
    return S @ zg, zg, st


@pytest.mark.parametrize("form", ["saved", "scalefree", "reortho"])
@pytest.mark.parametrize("case", R.CASES_B, ids=lambda c: c.name)
def test_lanczos_vectors(case, form, monkeypatch):
    """saved: z accumulated by k_multi_axpy(+1) from V; scalefree: the recurrence replayed, z += s r_j by k_axpy_const.  The twin's vectors go
    through the same Z S^T route (numpy.linalg.eigh), so the tolerance carries that route's cost.  spmv_kernel = 1: the product kernel that sums in
    a fixed order, so that the replayed recurrence and coeffs() are the run S was computed from, bit for bit."""
    tform = FORMS[form][2]
    bd = R.case_bundle(case, tform)
    at, bt, Vt = bd["twins"][tform]
    Vt_route = R.ritz_route(at, bt, Vt, R.numpy_eigh)
    _, (_, _, tol_v) = R.case_tolerances(case, tform, twin_vectors=Vt_route)
    H, init, K = bd["H"], bd["init"], case.K
    Vr = bd["ref"][2]
    with _engine(H, K, form, monkeypatch, spmv_kernel=1) as e:
        Vg, _, st = _engine_vectors(e, init, K)
        assert st["vectors_saved"] == (0 if form == "scalefree" else 1)
    dv = np.array([float(np.sqrt(np.sum(np.abs(Vg[j].astype(Vr[j].dtype) - Vr[j]) ** 2))) for j in range(K)])
    _report("B", "%s %s vectors" % (case.name, form), float((dv / tol_v).max()))
    assert np.all(dv <= tol_v), dv / tol_v
    if form == "reortho":
        Vtm = np.array(Vt_route)
        twin_fig = np.abs(Vtm.conj() @ Vtm.T - np.eye(K)).max()
        fig = np.abs(Vg.conj() @ Vg.T - np.eye(K)).max()
        bound = max(8.0 * twin_fig, 8.0 * R.EPS)
        _report("B", "%s reortho max|V^H V - I|" % case.name, fig / bound)
        assert fig <= bound, (fig, twin_fig)


@pytest.mark.parametrize("form", ["saved", "scalefree"])
@pytest.mark.parametrize("case", [R.case_a(257, False), R.case_a(2049, False)], ids=lambda c: c.name)
def test_kept_states_are_the_returned_vectors_bit_for_bit(case, form, monkeypatch):
    bd = R.case_bundle(case, FORMS[form][2])
    H, init, K = bd["H"], bd["init"], case.K
    assert H.n % 2 == 1
    with _engine(H, K, form, monkeypatch) as e:
        e.keep_states(2)
        _, zg, _ = e.lanczos(K, init=init, want_vectors=True)
        for k in range(2):
            assert np.array_equal(e.state(k).view(np.uint64), zg[k].view(np.uint64))
        assert np.linalg.norm(zg[0]) > 0.5


# ---- C: grid-stride trips -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,form", [(R.CASES_C[0], "scalefree"), (R.CASES_C[0], "saved"), (R.CASES_C[0], "reortho"), (R.CASES_C[1], "scalefree"),
                                       (R.CASES_C[1], "reortho")], ids=lambda v: v if isinstance(v, str) else v.name)
def test_second_trip_of_the_capped_grid(case, form, monkeypatch):
    """blas_blocks caps at 2048 blocks of 256 lanes: lengths beyond 2048 * 256 double2 take a second grid-stride trip"""
    n2 = case.n if case.cplx else (case.n + 1) // 2
    assert n2 > 2048 * 256
    _run_decomposition("C", case, form, monkeypatch)


# ---- D: the streamed pass --------------------------------------------------------------------------------------------------------------------------
def test_streamed_unrolled_pass_beyond_the_cache_switch(monkeypatch):
    """Real diagonal matrix, n = 16 777 216 + 2051: odd, 2 x n2 x 16 B beyond the 256 MiB switch, most lanes take the four-way unrolled body once, the last
    ones the scalar tail loop.  Long double at this length would take the test past a few seconds, so this one case compares against the float64
    normalised twin, with the derived bound (j+1) (log2 n + nnz_max + 4) eps |H|_inf (tree summation of n terms plus one row's products).  That twin
    against long double, measured once on the CPU for this input: |a - a_ld| <= 1.4e-4 and |b - b_ld| <= 0.101 of the bound (steps 0..2:
    b 0.100, 0.041, 0.001), below one eighth."""
    case = R.CASE_D
    bd = R.bundle(case.name, lambda: R.build(case), lambda: R.init_of(case), case.K, ("normalised",), with_reference=False)
    H, init = bd["H"], bd["init"]
    at, bt, _ = bd["twins"]["normalised"]
    bound = R.streamed_bound(H, case.K)
    with _engine(H, case.K, "scalefree", monkeypatch) as e:
        ag, bg, st = e.decomposition(init)
    assert st["vectors_saved"] == 0
    _check_coeffs("D", "%s scalefree" % case.name, H, ag, bg, at.astype(LD), bt.astype(LD), bound, bound)


# ---- E: product-basis forms --------------------------------------------------------------------------------------------------------------------------
def _pb_rows(name):
    from math import comb
    L, nup, ndown = R.pb_case(name)[:3]
    return comb(L, nup) * comb(L, ndown)


def _pb_bundle(name, tform):
    """reference (H = oracle.hubbard_csr of the same model), twins and tolerances of a product-basis case"""
    bd = R.bundle("E_" + name, lambda: R.pb_matrix(name), lambda: R.start_vector(_pb_rows(name), False, R.SEED_E), R.K_E, R.APPLICABLE[tform])
    return bd, R.tolerances(bd["H"], bd["ref"], [bd["twins"][f] for f in R.APPLICABLE[tform]])


def test_product_basis_cases_are_the_suites_own():
    from test_gpu_parity import PB_CASES
    for name in ("open_chain_L12", "disorder"):
        for mine, theirs in zip(R.pb_case(name), PB_CASES[name]()):
            assert np.array_equal(mine, theirs)


@pytest.mark.parametrize("save", [0, 1])
@pytest.mark.parametrize("name", ["open_chain_L12", "disorder"])
def test_coefficients_product_basis(name, save, monkeypatch):
    """open_chain_L12: the chained step (k_b2_from_w's derived norm, the deferred axpy riding in the next product); disorder: the three-kernel
    scale-free step (pb_combine_axpy, k_pb_reduce_a, k_pb_dq); save_vectors = 1: the normalised recurrence on pitched vectors"""
    chained = name == "open_chain_L12"
    tform = "normalised" if save else ("derived_norm" if chained else "scalefree")
    bd, (tol_a, tol_b, _) = _pb_bundle(name, tform)
    H, init = bd["H"], bd["init"]
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")
    monkeypatch.delenv("LPP_NO_SCALE_FREE", raising=False)
    with LanczosEngine(max_steps=R.K_E, eps=0.0, save_vectors=save) as e:
        e.assemble_hubbard(*R.pb_case(name))
        lay = e.layout()
        assert lay["kernel"] == 4 and e.rows() == H.n
        if chained:
            assert lay["chained_step"] == 1, lay
        else:
            assert lay["diagonal_plain"] == 1 and lay["chained_step"] == 0, lay
        ag, bg, st = e.decomposition(init)
        assert st["vectors_saved"] == save
    ar, br, _ = bd["ref"]
    _check_coeffs("E", "%s save_vectors=%d" % (name, save), H, ag, bg, ar, br, tol_a, tol_b)


def test_ritz_vector_through_the_second_pass_of_the_chained_step(monkeypatch):
    """computeAllStatesBelow(1, want_vectors=True) without kept vectors on the chained engine: the recurrence is replayed and every step materialises
    r_j (pb_materialise) before k_axpy_const adds it.  z against V_ref s, s from the engine's own coefficients; tolerance sum_j |s_j| tol_v[j]."""
    name = "open_chain_L12"
    bd, (_, _, tol_v) = _pb_bundle(name, "derived_norm")
    H, init, K = bd["H"], bd["init"], R.K_E
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")
    monkeypatch.delenv("LPP_NO_SCALE_FREE", raising=False)
    with LanczosEngine(max_steps=K, eps=0.0, save_vectors=0) as e:
        e.assemble_hubbard(*R.pb_case(name))
        assert e.layout()["chained_step"] == 1
        ag, bg, _ = e.decomposition(init)  # the chained pass, whose coefficients the solve diagonalises (the replay runs the three-kernel step: coeffs() after it differ in the last bits)
        eg, zg, st = e.lanczos(1, init=init, want_vectors=True)
        assert st["steps"] == K and st["vectors_saved"] == 0
    w, S = tridiag_lowest(ag, bg[:-1], 1, vectors=True)
    assert abs(w[0] - eg[0]) <= 1e-12 * abs(eg[0])
    s = S[:, 0]
    Vr = bd["ref"][2]
    zr = np.zeros(H.n, LD)
    for j in range(K):
        zr += LD(s[j]) * Vr[j]
    dev = float(np.sqrt(np.sum((zg[0].astype(LD) - zr) ** 2)))
    tol = float(np.sum(np.abs(s) * tol_v))
    _report("E", "%s Ritz vector, second pass" % name, dev / tol)
    assert dev <= tol, (dev, tol)
