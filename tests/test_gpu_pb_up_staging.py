"""The chained in-block kernel (k_pb_up<CHAIN>) at the edges of its staging.

A block's row of w goes into the LDS window with 16-byte global-to-LDS loads, the old vector's row into registers -- seven pairs
of doubles per thread (six where the look-ahead is deepest), requested one block AHEAD from the tail of the slice loop --, and every
thread corrects in LDS the pairs its own lane has loaded.  What decides the path is the row length N_up (pairs per thread =
N_up / 2 / 1024) and how often a workgroup walks its block loop (the early request runs once per block after the first):

    L = 8,  (4, 2):   70 positions   most threads have no pair at all, 28 blocks
    L = 12, (6, 4):  924             fewer than one pair per thread; 495 blocks: the block loop is walked at least twice, so the
                                     request from the tail runs at least once in every workgroup
    L = 14, (7, 2): 3432             between one and two pairs, 91 blocks
    L = 16, (8, 1) and (8, 2): 12870 6.3 pairs, the flagship row; 16 and 120 blocks
    L = 20, (5, 1): 15504            7.6 pairs: the staging's second trip, 20 blocks
    L = 10, (5, 3), complex hoppings: 252 positions, four value groups -- the instantiation for any number of groups, whose
                                     slice loop has no peeled tail (it asks behind the loop); 120 blocks
    L = 12, (6, 2):  924             66 blocks on a GPU with more CUs: every workgroup has exactly one block, nothing to ask for

Checked against the CPU oracle as in tests/test_gpu_pb_up_waits.py, with its tolerances: the product x += H y, the chained
coefficients from a GIVEN start vector and the lowest Ritz value.  Sectors of more than 2e5 states run a fixed 16 steps (eps = 0 on
both sides: the step count is the limit), which keeps a case at a few seconds and the comparison clear of the late, ill-conditioned
steps of a converged run; the small ones run to convergence.
"""
from math import comb

import numpy as np
import pytest
import torch  # (loaded before the engine library, so that both use one HIP runtime -- INTEGRATION.md)

import oracle
from helpers import chain, rel, square
from lanczosplusplus_amd import LanczosEngine
from test_gpu_parity import E_TOL, SPMV_TOL

pytestmark = pytest.mark.gpu

FIXED_STEPS = 16


def _phases(L):
    """a ring with a Peierls phase on every bond"""
    up = np.triu(np.ones((L, L)), 1) > 0
    hop = chain(L, -1.0, True).astype(complex) * np.where(up, np.exp(0.37j), np.exp(-0.37j))
    assert np.allclose(hop, hop.conj().T)
    return hop


# name: (L, n_up, n_down, hopping matrix, run a fixed number of steps); U = 4 on every site
CASES = {
    "no_pair_for_most_threads": (8, 4, 2, chain(8, -1.0, pbc=True), False),
    "under_one_pair_block_loop_twice": (12, 6, 4, chain(12, -1.0, pbc=True), True),
    "one_to_two_pairs": (14, 7, 2, chain(14, -1.0, pbc=True), True),
    "flagship_row_16_blocks": (16, 8, 1, square(4, 4, -1.0, pbc=True), True),
    "flagship_row_120_blocks": (16, 8, 2, square(4, 4, -1.0, pbc=True), True),
    "second_trip": (20, 5, 1, chain(20, -1.0, pbc=True), True),
    "complex_hoppings_any_groups": (10, 5, 3, _phases(10), False),
    "more_cus_than_blocks": (12, 6, 2, chain(12, -1.0, pbc=True), False),
}


class _Ref:
    """oracle results of a case, computed once per module and left unchanged"""

    def __init__(self, name):
        L, nup, ndn, hop, fixed = CASES[name]
        self.L, self.nup, self.ndn, self.hop = L, nup, ndn, hop
        self.U = np.full(L, 4.0)
        A = oracle.hubbard_csr(L, nup, ndn, hop, self.U)
        assert A.nrows == comb(L, nup) * comb(L, ndn)
        self.cplx = bool(A.is_complex)
        self.kw = dict(max_steps=FIXED_STEPS, min_steps=FIXED_STEPS, eps=0.0) if fixed else {}
        self.init = oracle.fill_random(A.nrows, 1234, self.cplx)
        self.x = oracle.fill_random(A.nrows, 5, self.cplx)
        self.y = oracle.fill_random(A.nrows, 6, self.cplx)
        self.xo = oracle.spmv_acc(A, self.x.copy(), self.y, nthreads=0)
        self.eo, _, self.so = oracle.lanczos_solve(A, self.init, want_vectors=False, nthreads=0, **self.kw)
        self.steps_o, ao, bo, _, _ = oracle.lanczos_decomposition(A, self.init, nthreads=0, **self.kw)
        self.ao, self.bo = np.asarray(ao), np.asarray(bo)
        for v in (self.init, self.x, self.y, self.xo, self.ao, self.bo):
            v.flags.writeable = False


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Ref(name)
        return cache[name]

    return get


def _engine(r):
    e = LanczosEngine(dtype="c128" if r.cplx else "f64", save_vectors=0, **r.kw)
    try:
        e.assemble_hubbard(r.L, r.nup, r.ndn, r.hop, r.U)
        lay = e.layout()
        assert lay["kernel"] == 4, lay  # the product-basis layout, not a fall-back to the general one
        assert lay["chained_step"] == 1, lay
        assert lay["pieces"] == 1 and lay["segments"] == 0, lay  # the row in ONE LDS window: k_pb_up, not the kernels for longer rows
    except BaseException:
        e.__exit__(None, None, None)
        raise
    return e


@pytest.mark.parametrize("name", list(CASES))
def test_chained_in_block_kernel_at_the_edges_of_its_staging(refs, name, monkeypatch):
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")  # below the size from which the layout is chosen by itself
    r = refs(name)
    if name == "more_cus_than_blocks":
        assert comb(r.L, r.ndn) < torch.cuda.get_device_properties(0).multi_processor_count
    with _engine(r) as e:
        xg = e.matrixVectorProduct(r.x.copy(), r.y.copy())
        print("%s: product rel %.3e" % (name, rel(xg, r.xo)))
        assert rel(xg, r.xo) < SPMV_TOL
        ag, bg, _ = e.decomposition(r.init.copy())
        print("%s: steps %d (oracle %d)" % (name, len(ag), r.steps_o))
        assert len(ag) == r.steps_o
        print("%s: alpha rel %.3e, beta rel %.3e" % (name, rel(ag, r.ao), rel(bg, r.bo)))
        assert rel(ag, r.ao) < 1e-8 and rel(bg, r.bo) < 1e-8
        eg, _, st = e.lanczos(1, want_vectors=False)
        print("%s: E0 %.14f (oracle %.14f)" % (name, eg[0], r.eo[0]))
        assert abs(eg[0] - r.eo[0]) <= E_TOL * abs(r.eo[0])
        assert st["steps"] == r.so


def test_chained_coefficients_are_bitwise_reproducible_with_the_second_trip(refs, monkeypatch):
    """two fresh engines on the row that takes the staging's second trip: r_next is formed once per pair, whichever trip loads it"""
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")
    r = refs("second_trip")
    runs = []
    for _ in range(2):
        with _engine(r) as e:
            ag, bg, _ = e.decomposition(r.init.copy())
        runs.append((np.ascontiguousarray(ag).view(np.uint64), np.ascontiguousarray(bg).view(np.uint64)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
