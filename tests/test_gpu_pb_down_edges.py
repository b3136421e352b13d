"""-m gpu: the coupling kernel (k_pb_down, lpp_pb_kernels.h) at the edges of its own structure, against long double.

A workgroup of the kernel owns a range of blocks, walks it in tasks of 8 blocks per wave (handed out by an LDS counter or in fixed shares), and a
task gathers its coupling lists in chunks of 4 places: a prologue of two chunks, then a loop unrolled by three that re-issues into the buffers it
has just consumed.  The cases (lanczos_reference.PB_DOWN_CASES; Hubbard, U = 4, no potentials) are the smallest sectors at which those edges
differ -- what each one reaches is asserted below from the device's own CU count (test_the_cases_reach_their_edges) and, for 256 CUs, without
a GPU in tests/test_lanczos_reference_host.py and lanczosplusplus_amd/host/test_pb_plan.cpp:

    all-to-all +-1 (seed 3), (8,4,1)    8 blocks, 1 per workgroup   lists of 7: 2 chunks, the prologue alone; one valid sub-row of 8 per task; most
                                                                     workgroups own nothing; 5 panels for 8 groups
    all-to-all +-1 (seed 3), (8,4,3)    56 blocks, 2                lists of 15: 4 chunks, the first re-issue into the first buffer
    all-to-all +-1 (seed 3), (10,3,5)   252 blocks, 8               lists of 25: 7 chunks, the loop's second back edge; exactly one full task per
                                                                     workgroup, the last one half a task; 28 places in rows of 28 words
    all-to-all +-1 (seed 11), (12,2,6)  924 blocks, 29              lists of 36: 9 chunks, a third trip; a padded last task (29 = 3 * 8 + 5)
    ring + 0.5 second neighbour, (11,5,4)  330 blocks, 11           lists of 4 to 14 inside one task (filler places), four coupling values, 29 panels:
                                                                     the pacing waits, groups of 4 and of 3 panels
    ring, (14,2,4)                      1001 blocks, 32             two rounds of 16, the last workgroup (9 blocks) with an empty second round
    ring, (15,2,6)                      5005 blocks, 157            20 tasks against 16 waves: the fixed shares take a second turn
    Peierls ring, (11,5,4)              330 blocks, 11, complex     the complex kernel in every form

and LPP_PB_DOWN_GRID=8 puts all 924 blocks of the fourth case into one workgroup per group: 116 tasks per step (the second trip of the task sums'
fold), rounds in units of 64 blocks (512 + 412), the image copy of such a range.

Every (case, form) is held to bounds in which nothing comes from the engine:
  * the structure (once per case): get_csr() is the oracle's CSR bit for bit;
  * the product x = x0 + H y, row by row, against the same product in long double: lanczos_reference.product_bound, the first-order forward bound
    (nnz_i + 4) 2^-53 (|x0_i| + sum_j |H_ij| |y_j|) of ANY double-precision evaluation of the row ((2 nnz_i + 6) 2^-53 with moduli for complex rows);
  * the coefficients a_j, b_j of the first K steps from a given start vector against the long-double recurrence, step by step, with the rule of
    tests/test_gpu_lanczos_steps.py (lanczos_reference.tolerances: max(8 |twin - reference|, 4 eps |H|_inf)): the chained step (k_pb_down<RMW>, whose
    task sums feed nothing but these coefficients) under the derived-norm set of twins, the three-kernel step of the forms without it under the
    scale-free set.  eps = 0: the step count is the limit on both sides; 16 steps, 8 for sectors above 2e5 states.
The input conditions of every case are asserted in tests/test_lanczos_reference_host.py.  Each check prints its largest deviation / bound ratio
(pytest -s or -rP; DESIGN.md section 3 records them as group F)."""
import re
from math import comb

import numpy as np
import pytest
import torch  # loaded before the engine library, so that both use one HIP runtime -- INTEGRATION.md

import lanczos_reference as R
import oracle
from lanczosplusplus_amd import LanczosEngine

pytestmark = pytest.mark.gpu

LD = np.longdouble
CASES = list(R.PB_DOWN_CASES)
WIDE = dict(LPP_PB_PIECE_ROWS="320", LPP_PB_WIDE="1", LPP_PB_BIG2="0")  # the switch set of the "wide" form of tests/test_gpu_parity.py
# form -> (environment, chained step, (down tasks, chained counter form, pacing dropped) of the LPP_VERBOSE line)
#   chained step on: the product runs the plain kernel, the coefficients the chained one (k_pb_down<RMW>)
FORMS = {
    "default": ({}, 1, (1, 1, 1)),  # plain: counter tasks, no pacing; chained: counter tasks, u lines touched ahead, pacing dropped
    "tasks0": (dict(LPP_PB_DOWN_TASKS="0"), 1, (0, 1, 1)),  # plain: fixed shares, paced
    "pf0": (dict(LPP_PB_DOWN_PF="0"), 1, (1, 0, 0)),  # chained: fixed shares, paced (the complex case: k_pb_down<1024, true, false, true, false>)
    "chain_pace1": (dict(LPP_PB_CHAIN_PACE="1"), 1, (1, 1, 0)),  # chained: counter tasks, paced
    "rounds2": (dict(LPP_PB_DOWN_ROUNDS="2"), 0, (1, 1, 1)),  # two LDS images per panel, copied from the prepared buffer
    "rounds2_rebuilt": (dict(LPP_PB_DOWN_ROUNDS="2", LPP_PB_DOWN_IMAGE="0"), 0, (1, 1, 1)),  # ... rebuilt from the lists
    "wide": (WIDE, 0, (1, 1, 1)),  # 64-bit addresses from line numbers
    "grid8": (dict(LPP_PB_DOWN_GRID="8"), 1, (1, 1, 1)),  # one workgroup per group
    "grid8_rounds2": (dict(LPP_PB_DOWN_GRID="8", LPP_PB_DOWN_ROUNDS="2"), 0, (1, 1, 1)),
}
RUNS = ([(c, f) for f in ("default", "tasks0", "pf0") for c in CASES]
        + [(c, "chain_pace1") for c in ("ttp_ring_11_5_4", "peierls_11_5_4")]  # the two with enough panels to wait
        + [(c, f) for f in ("rounds2", "rounds2_rebuilt") for c in ("ring_14_2_4", "a2a_12_2_6")]
        + [(c, "wide") for c in ("a2a_10_3_5", "peierls_11_5_4")]
        + [("a2a_12_2_6", f) for f in ("grid8", "grid8_rounds2")])
SWITCHES = sorted({k for env, _, _ in FORMS.values() for k in env} | {"LPP_PB_CHAIN", "LPP_PB_PACE", "LPP_PB_PARTS", "LPP_PB_ORDER_WINDOW", "LPP_PB_PERM", "LPP_PB_SEG", "LPP_NO_SCALE_FREE"})


def _report(tag, what, ratio):
    print("[lanczos-steps] group F %s: %s, largest deviation / bound = %.3f" % (tag, what, ratio))


class _Ref:
    """everything of a case that does not come from the engine, computed once per module and left unchanged"""

    def __init__(self, name):
        self.name = name
        self.model = R.pb_case(name)
        self.L, self.nup, self.ndn, self.hop = self.model[:4]
        self.cplx = R.pb_is_complex(name)
        self.K = R.pb_steps(name)
        self.A = oracle.hubbard_csr(*self.model)
        assert self.A.nrows == R.pb_rows(name) and bool(self.A.is_complex) == self.cplx
        self.H = R.Csr(self.A.rowptr, self.A.colind, self.A.values, self.A.nrows)
        self.x0, self.y = oracle.fill_random(self.H.n, 5, self.cplx), oracle.fill_random(self.H.n, 6, self.cplx)
        self.xr, self.bound = R.product_reference(self.H, self.x0, self.y), R.product_bound(self.H, self.x0, self.y)
        self.lens = R.coupling_list_lengths(self.L, self.ndn, self.hop)
        for v in (self.x0, self.y, self.xr, self.bound):
            v.flags.writeable = False

    def coefficients(self, tform):
        """reference, start vector and tolerances for a device form bounded by the twin set `tform`"""
        bd = R.bundle("F_" + self.name, lambda: self.H, lambda: R.pb_start(self.name), self.K, R.APPLICABLE[tform])
        return bd, R.tolerances(bd["H"], bd["ref"], [bd["twins"][f] for f in R.APPLICABLE[tform]])


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Ref(name)
        return cache[name]

    return get


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _geometry(r, env):
    return R.down_geometry(comb(r.L, r.ndn), int(r.lens.max()), _cus(), grid=int(env["LPP_PB_DOWN_GRID"]) if "LPP_PB_DOWN_GRID" in env else None,
                           rounds=int(env["LPP_PB_DOWN_ROUNDS"]) if "LPP_PB_DOWN_ROUNDS" in env else None)


def _engine(r, form, monkeypatch, capfd):
    """a fresh engine in `form`; the switches are read when the layout is built.  Asserts the layout's own account of the form and, from the lines the
    build prints under LPP_VERBOSE, the launch forms and the coupling kernel's geometry against its restatement (lanczos_reference.down_geometry)"""
    env, chained, flags = FORMS[form]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")
    monkeypatch.setenv("LPP_VERBOSE", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = _geometry(r, env)
    capfd.readouterr()
    e = LanczosEngine(dtype="c128" if r.cplx else "f64", max_steps=r.K, eps=0.0, save_vectors=0)
    try:
        e.assemble_hubbard(*r.model)
        err = capfd.readouterr().err
        lay = e.layout()
        assert lay["kernel"] == 4 and e.rows() == r.H.n, lay
        assert lay["chained_step"] == chained and lay["coupling_rounds"] == g["rounds"] and lay["coupling_parts"] == 1, lay
        assert form == "wide" or lay["pieces"] == 1, lay  # (the wide form cuts the rows into pieces of at most 320 positions)
        launch = re.findall(r"lpp: product-basis launch forms: chain (\d+), down tasks (\d+), chained counter form (\d+), pacing dropped (\d+), lazy exchange (\d+)", err)
        assert launch and all(tuple(map(int, ln)) == (chained,) + flags + (0,) for ln in launch), (launch, err[-2000:])
        grid = re.findall(r"lpp: coupling kernel grid (\d+) \((\d+) workgroups per group, (\d+) blocks each in (\d+) rounds of (\d+)\)", err)
        want = (g["grid"], g["slots"], g["ids_per_wg"], g["rounds"], g["ids_per_round"])
        assert grid and all(tuple(map(int, ln)) == want for ln in grid), (grid, want)
    except BaseException:
        e.__exit__(None, None, None)
        raise
    return e


def test_the_cases_are_the_sibling_suites_matrices():
    from test_gpu_pb_up_staging import _phases
    from test_gpu_pb_up_waits import _all_to_all
    for L, seed in ((8, 3), (10, 3), (12, 11)):
        assert np.array_equal(R.all_to_all(L, [1.0], seed), _all_to_all(L, [1.0], seed))
    assert np.array_equal(R.peierls_ring(11), _phases(11))
    for name in CASES:
        L, nup, ndn, hop, U, V = R.pb_case(name)
        assert np.array_equal(U, np.full(L, 4.0)) and not V.any() and np.allclose(hop, hop.conj().T) and not np.diag(hop).any()


def test_the_cases_reach_their_edges(refs):
    """what every case is there for, from this device's CU count (the figures of the module's docstring assume 256 CUs: 32 workgroups per group)"""
    slots = (_cus() & ~7) // 8
    assert _cus() >= 8
    geo = {}
    for name in CASES:
        r = refs(name)
        n_blk = comb(r.L, r.ndn)
        assert len(r.lens) == n_blk
        geo[name] = (n_blk, -(-n_blk // slots), int(r.lens.min()), int(r.lens.max()), (comb(r.L, r.nup) * (2 if r.cplx else 1) + 15) // 16)
    n_blk, ids, lo, hi, panels = geo["a2a_8_4_1"]
    assert ids == 1 and n_blk < slots and (lo, hi) == (7, 7) and panels < 8  # workgroups without a block, one valid sub-row per task, 2 chunks, groups without a panel
    n_blk, ids, lo, hi, panels = geo["a2a_8_4_3"]
    assert lo == hi == 15 and ids >= 1  # 4 chunks: the first re-issue (ch + 3 < n4)
    n_blk, ids, lo, hi, panels = geo["a2a_10_3_5"]
    assert ids == 8 and n_blk % 8 == 4 and lo == hi == 25 and R.down_geometry(n_blk, hi, _cus())["rowcap"] == 28  # one full task; half a task; 7 chunks: the second back edge
    n_blk, ids, lo, hi, panels = geo["a2a_12_2_6"]
    assert lo == hi == 36 and ids % 8 != 0 and ids > 16  # 9 chunks: a third trip; a padded last task, several tasks
    n_blk, ids, lo, hi, panels = geo["ttp_ring_11_5_4"]
    assert (lo, hi) == (4, 14) and ids >= 8 and panels == 29 and panels >= 3 * 8  # filler places inside a task; waits (p >= grp + 16); groups of 4 and of 3 panels
    lens = refs("ttp_ring_11_5_4").lens  # a workgroup's blocks by decreasing list length (its range is shorter than a sorting window): the first task's lists differ
    assert ids <= 64 and any(len(set(sorted(lens[w:w + ids], reverse=True)[:8])) > 1 for w in range(0, n_blk, ids))
    n_blk, ids, lo, hi, panels = geo["ring_14_2_4"]
    g = R.down_geometry(n_blk, hi, _cus(), rounds=2)
    last = n_blk - (slots - 1) * ids
    assert g["rounds"] == 2 and 0 < last <= g["ids_per_round"] < ids  # the last workgroup's second round is empty
    n_blk, ids, lo, hi, panels = geo["ring_15_2_6"]
    assert (ids + 7) // 8 > 16  # more tasks than waves: a second turn of the fixed shares
    n_blk, ids, lo, hi, panels = geo["peierls_11_5_4"]
    assert panels >= 3 * 8 and refs("peierls_11_5_4").cplx
    # the forced grid: everything in one workgroup per group
    n_blk, ids, lo, hi, panels = geo["a2a_12_2_6"]
    g = R.down_geometry(n_blk, hi, _cus(), grid=8)
    assert (g["slots"], g["ids_per_wg"], g["rounds"]) == (1, 924, 1) and (924 + 7) // 8 > 64 and g["lds_pf"] <= 150 * 1024  # fold's second trip; the counter form still fits
    g = R.down_geometry(n_blk, hi, _cus(), grid=8, rounds=2)
    assert (g["rounds"], g["ids_per_round"]) == (2, 512)  # units of 64 blocks: 512, then 412


@pytest.mark.parametrize("name", CASES)
def test_structure_is_the_oracles_bit_for_bit(refs, name, monkeypatch, capfd):
    r = refs(name)
    with _engine(r, "default", monkeypatch, capfd) as e:
        rp, ci, va = e.get_csr()
    assert np.array_equal(rp, r.A.rowptr) and np.array_equal(ci, r.A.colind)
    assert np.array_equal(np.ascontiguousarray(va).view(np.uint64), np.ascontiguousarray(r.A.values).view(np.uint64))


@pytest.mark.parametrize("name,form", RUNS, ids=["%s-%s" % cf for cf in RUNS])
def test_product_elementwise_and_coefficients_per_step(refs, name, form, monkeypatch, capfd):
    from test_gpu_lanczos_steps import _check_coeffs
    r = refs(name)
    chained = FORMS[form][1]
    tform = "derived_norm" if chained else "scalefree"
    bd, (tol_a, tol_b, _) = r.coefficients(tform)
    ar, br, _ = bd["ref"]
    tag = "%s %s" % (name, form)
    with _engine(r, form, monkeypatch, capfd) as e:
        xg = e.matrixVectorProduct(r.x0.copy(), r.y.copy())
        ag, bg, st = e.decomposition(bd["init"].copy())
        assert st["vectors_saved"] == 0
    dev = np.abs(xg.astype(r.xr.dtype) - r.xr)
    ratio = dev / r.bound
    _report(tag, "product", float(ratio.max()))
    failed = []  # both checks run, so that a failure of the product does not hide what the coefficients say
    if not np.all(dev <= r.bound):
        failed.append(("product", "row %d" % int(np.argmax(ratio)), "deviation / bound %.3g" % float(ratio.max()), "%d rows beyond the bound" % int((dev > r.bound).sum())))
    try:
        _check_coeffs("F", "%s %s" % (tag, "chained step" if chained else "three-kernel step"), r.H, ag, bg, ar, br, tol_a, tol_b)
    except AssertionError as err:
        failed.append(("coefficients", (str(err).splitlines() or ["step count"])[0][:300]))
    assert not failed, (tag, failed)


def test_coefficients_are_bitwise_reproducible_with_every_block_in_one_workgroup(refs, monkeypatch, capfd):
    """two fresh engines, 116 tasks per step handed by the counter to whichever wave asks first: the fold of the task sums makes that invisible"""
    r = refs("a2a_12_2_6")
    init = R.pb_start(r.name)
    runs = []
    for _ in range(2):
        with _engine(r, "grid8", monkeypatch, capfd) as e:
            ag, bg, _ = e.decomposition(init.copy())
        assert len(ag) == r.K
        runs.append((np.ascontiguousarray(ag).view(np.uint64), np.ascontiguousarray(bg).view(np.uint64)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
