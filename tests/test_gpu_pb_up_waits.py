"""The in-block kernel (k_pb_up) at the edges of its slice loop and of its block loop.

The kernel keeps the template words of two slices per wave in flight (64 rows make a slice, 16 waves per workgroup) and orders
its block loop with barriers that cover LDS only.  The shapes below are the smallest ones at which the edges of that structure
differ: a wave without a slice, a wave with one slice, with one and with two, with an odd and an even number, a partial last
slice, one block per workgroup and several, lists longer than the look-ahead in the unrolled (two value groups) and in the plain
(more than two) loop, a single value group.  Every case is checked against the CPU oracle the way tests/test_gpu_parity.py does:
the product x += H y (the plain form of the kernel), the Lanczos coefficients from a GIVEN start vector (the chained form: its
first step has no old row to subtract, the steps after it do) and the lowest Ritz value.

The sign patterns of the all-to-all hoppings are fixed seeds chosen for a WELL-CONDITIONED reference: the oracle's own coefficients,
run again from the start vector with its last bit perturbed, must agree to better than 1e-12 over the whole run (seeds 1-5 at
L = 10 give 2e-14 to 5e-14 in 46-76 steps).  Seed 7 at L = 10 does not qualify: its run takes 123 steps and the oracle disagrees with
itself by 7e-5 from step 113 on, so no product kernel, however exact, can meet rel < 1e-8 there.
"""
from math import comb

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before the engine library, so that both use one HIP runtime -- INTEGRATION.md)

import oracle
from helpers import chain, rel
from lanczosplusplus_amd import LanczosEngine
from test_gpu_parity import E_TOL, SPMV_TOL

pytestmark = pytest.mark.gpu


def _all_to_all(L, magnitudes, seed):
    """symmetric hopping between every pair of sites, magnitudes drawn from `magnitudes`, signs mixed"""
    rng = np.random.default_rng(seed)
    m = np.zeros((L, L))
    for i in range(L):
        for j in range(i + 1, L):
            m[i, j] = m[j, i] = rng.choice(magnitudes) * rng.choice([-1.0, 1.0])
    return m


# name: (L, n_up, n_down, hopping matrix); U = 4 on every site.  N_up = C(L, n_up) is the row length, C(L, n_down) the number of blocks
CASES = {
    # 70 rows = 2 slices (the second one 6 rows): 14 of the 16 waves have no slice at all
    "wave_without_slice": (8, 4, 2, chain(8, -1.0, pbc=True)),
    # 1716 rows = 26 full slices + 52 rows: waves with two slices and waves with one (the second of the pair out of range), a partial
    # last slice, a row that is no multiple of 16; 78 blocks: one block per workgroup, fewer blocks than CUs
    "pair_half_empty": (13, 6, 2, chain(13, -1.0, pbc=True)),
    # 924 rows = 15 slices: every wave but one has exactly one slice; 495 blocks: each workgroup walks the block loop at least twice
    "one_slice_per_wave_many_blocks": (12, 6, 4, chain(12, -1.0, pbc=True)),
    # up to 25 entries per row in two value groups (+1, -1): lists longer than the look-ahead, the unrolled loop
    "long_lists_two_groups": (10, 5, 3, _all_to_all(10, [1.0], 3)),
    # up to 36 entries per row in two value groups: more than the 32 slots the look-ahead of both groups holds
    "longer_lists_two_groups": (12, 6, 2, _all_to_all(12, [1.0], 11)),
    # magnitudes 1 and 0.5: four value groups, the loop for any number of groups
    "long_lists_four_groups": (10, 5, 3, _all_to_all(10, [1.0, 0.5], 7)),
    # open chain, nearest-neighbour hopping of one sign: no fermion sign inside a species, one value group
    "one_value_group": (12, 6, 3, chain(12, -1.0)),
    # the same edges at longer rows: 792 rows = 13 slices (the last one 24 rows), three waves without a slice ...
    "waves_without_slice_792": (12, 5, 2, chain(12, -1.0, pbc=True)),
    # ... and the four value groups of mixed magnitudes at up to 36 entries per row
    "longer_lists_four_groups": (12, 6, 2, _all_to_all(12, [1.0, 0.5], 11)),
    # 3432 rows = 54 slices: three or four slices per wave, one trip through the two-slice loop, then one or two slices behind it
    "loop_once": (14, 7, 2, chain(14, -1.0, pbc=True)),
    # 6435 rows = 101 slices: six or seven slices per wave, the loop's back edge taken
    "loop_back_edge": (15, 7, 1, chain(15, -1.0, pbc=True)),
}


class _Ref:
    """oracle results of a case, computed once per module and left unchanged"""

    def __init__(self, name):
        L, nup, ndn, hop = CASES[name]
        self.L, self.nup, self.ndn, self.hop = L, nup, ndn, hop
        self.U = np.full(L, 4.0)
        A = self.A = oracle.hubbard_csr(L, nup, ndn, hop, self.U)
        assert A.nrows == comb(L, nup) * comb(L, ndn)
        self.init = oracle.fill_random(A.nrows, 1234)
        self.x = oracle.fill_random(A.nrows, 5)
        self.y = oracle.fill_random(A.nrows, 6)
        self.xo = oracle.spmv_acc(A, self.x.copy(), self.y)
        self.eo, _, self.so = oracle.lanczos_solve(A, self.init, want_vectors=False)
        self.steps_o, self.ao, self.bo, _, _ = oracle.lanczos_decomposition(A, self.init)
        self.ao, self.bo = np.asarray(self.ao), np.asarray(self.bo)
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


def _engine(r, **kw):
    e = LanczosEngine(save_vectors=0, **kw)
    try:
        e.assemble_hubbard(r.L, r.nup, r.ndn, r.hop, r.U)
        lay = e.layout()
        assert lay["kernel"] == 4, lay  # the product-basis layout, not a fall-back to the general one
        assert lay["chained_step"] == 1, lay  # every case has down hops and few diagonal values: the chained step serves it
    except BaseException:
        e.__exit__(None, None, None)
        raise
    return e


@pytest.mark.parametrize("name", list(CASES))
def test_in_block_kernel_at_the_edges_of_its_loops(refs, name, monkeypatch):
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")  # below the size from which the layout is chosen by itself
    r = refs(name)
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


def test_first_chained_step_then_regular_steps(refs, monkeypatch):
    """Three steps from a given start vector: the first launch of the chained kernel has no previous vector (nothing to subtract,
    no old row read), the two after it have.  eps = 0: the step count is the limit on both sides."""
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")
    r = refs("pair_half_empty")
    steps_o, ao, bo, _, _ = oracle.lanczos_decomposition(r.A, r.init, max_steps=3, eps=0.0)
    with _engine(r, max_steps=3, min_steps=3, eps=0.0) as e:
        ag, bg, _ = e.decomposition(r.init.copy())
    print("first steps: alpha", ag, ao, "beta", bg, bo)
    assert len(ag) == steps_o
    assert rel(ag, ao) < 1e-8 and rel(bg, bo) < 1e-8


def test_chained_coefficients_are_bitwise_reproducible(refs, monkeypatch):
    """two fresh engines, the case whose workgroups walk the block loop several times: no result depends on which wave or block
    came first"""
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1")
    r = refs("one_slice_per_wave_many_blocks")
    runs = []
    for _ in range(2):
        with _engine(r) as e:
            ag, bg, _ = e.decomposition(r.init.copy())
        runs.append((np.ascontiguousarray(ag).view(np.uint64), np.ascontiguousarray(bg).view(np.uint64)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
