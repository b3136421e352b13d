"""Operator strings on the GPU: the whole product applied in one launch (apply_operator_string), many-point correlations and measure brackets in one
pass over bra and ket (many_point, measure), batching, physics pins on a ground state and the driver's -M / -m, against tests/many_point_reference.py."""
import os
import subprocess

import numpy as np
import pytest

import many_point_reference as mp
import obs_reference as ref
import oracle
from helpers import chain
from lanczosplusplus_amd import LanczosEngine, LppError, geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "lanczosplusplus_amd", "host", "lanczos")
GOLD = os.path.join(ROOT, "tests", "golden")
UP, DOWN = ref.UP, ref.DOWN

pytestmark = pytest.mark.gpu

# sizes: the L = 8 ring sectors of test_apply_operator (4900 and 3920 states, three kernel tiles); L = 5 (2,1): 50 states, an odd length, so the f64
# path ends in half a unit; L = 6 (3,0) and (0,3): one block, or N_up = 1
SECTORS = [(8, (4, 4)), (8, (4, 3)), (5, (2, 1)), (6, (3, 0)), (6, (0, 3))]

# sites below 5, so every string is valid for every L above
STRINGS = [
    [("c", 1, UP), ("cdagger", 3, UP)],
    [("cdagger", 2, DOWN), ("c", 0, DOWN)],
    [("c", 1, UP), ("c", 2, DOWN), ("cdagger", 4, DOWN), ("cdagger", 3, UP)],  # pair hopping
    [("c", 0, DOWN), ("c", 1, UP), ("cdagger", 0, DOWN), ("cdagger", 1, UP)],
    [("n", 0, UP), ("n", 1, UP), ("n", 2, UP)],
    [("n", 0, UP), ("n", 1, DOWN)],
    [("sz", 0, UP), ("sz", 1, UP)],
    [("sz", 1, UP), ("c", 1, UP), ("sz", 1, UP), ("cdagger", 1, UP), ("sz", 2, DOWN)],
    [("splus", 1, UP), ("sz", 1, UP), ("sminus", 3, UP)],
    [("c", 0, UP), ("n", 1, UP), ("cdagger", 2, DOWN)],  # ends in another sector
    [("splus", 0, UP), ("sz", 0, DOWN)],  # ends in another sector
    [("cdagger", 0, UP), ("cdagger", 1, UP), ("cdagger", 2, UP), ("cdagger", 3, UP), ("cdagger", 4, UP), ("n", 0, UP), ("c", 0, UP)],  # may leave [0, L]
    [("c", 0, UP), ("c", 1, UP), ("c", 2, UP), ("cdagger", 0, UP)],  # through (0,0) from (3,0)
]
MEASURES = [
    [("n", 0, UP, False), ("n", 1, DOWN, False)],
    [("c", 2, UP, True), ("c", 0, UP, False)],
    [("c", 1, DOWN, True), ("sz", 3, DOWN, False), ("c", 3, DOWN, False)],
    [("c", 3, UP, True), ("c", 4, DOWN, True), ("c", 2, DOWN, False), ("c", 1, UP, False)],
    [("sz", 0, UP, False), ("sz", 0, DOWN, False), ("identity", 2, UP, False), ("n", 1, UP, False)],
]


def _ring(L):
    return chain(L, -1.0, True)


# ---- 1. the string applied to a vector: every output element is one product ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("L,parts", SECTORS)
def test_apply_operator_string(dtype, L, parts):
    cplx = dtype == "c128"
    src = oracle.fill_random(mp.size(L, parts), 11, cplx)
    factor = (0.75 - 0.5j) if cplx else -1.25
    launched = 0
    with LanczosEngine(dtype=dtype) as e:
        for ops in STRINGS:
            want, new = mp.chain(ops, L, parts, src, factor)
            z, got_parts = e.apply_operator_string(ops, L, parts[0], parts[1], src, factor=factor)
            if want is None:
                assert z is None and got_parts is None, ops
                continue
            launched += 1
            assert got_parts == new, ops
            assert np.max(np.abs(z - want)) <= 1e-14 * np.max(np.abs(want)), ops
            idx, _, _ = mp.chain_action(ops, L, parts)
            untouched = np.ones(len(z), bool)
            untouched[idx[idx >= 0]] = False
            assert np.all(z[untouched] == 0), ops
            z2, _ = e.apply_operator_string(ops, L, parts[0], parts[1], src, factor=factor, out=z)  # z += ...
            assert np.max(np.abs(z2 - 2 * want)) <= 2e-14 * np.max(np.abs(want)) and np.all(z2[untouched] == 0), ops
        for vops in MEASURES:
            want = factor * mp.rahul_method(vops, L, parts, src)
            z, got_parts = e.apply_operator_string(vops, L, parts[0], parts[1], src, factor=factor, convention="measure")
            assert got_parts == parts
            assert np.max(np.abs(z - want)) <= 1e-14 * np.max(np.abs(want)), vops
            assert np.all(z[want == 0] == 0), vops
            launched += 1
    assert launched >= len(MEASURES) + 4


# ---- 2. brackets of random vectors --------------------------------------------------------------------------------------------------------------
def _bound(bra, ket):
    """the standard bound of a dot product of n terms in any order with Cauchy-Schwarz: n 2^-53 |bra| |ket|.  One wrong sign or index moves the sum
    by about 1/n of the norm product, far above it."""
    return len(bra) * 2.0 ** -53 * np.linalg.norm(bra) * np.linalg.norm(ket)


@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("L,parts", SECTORS)
def test_many_point_random_vectors(dtype, L, parts):
    cplx = dtype == "c128"
    n = mp.size(L, parts)
    bra, ket = oracle.fill_random(n, 5, cplx), oracle.fill_random(n, 6, cplx)
    with LanczosEngine(dtype=dtype) as e:
        got = e.many_point_of(STRINGS, L, parts[0], parts[1], bra, ket)
        assert got.dtype == (np.complex128 if cplx else np.float64) and len(got) == len(STRINGS)
        nonzero = 0
        for ops, g in zip(STRINGS, got):
            want = mp.many_point(ops, L, parts, bra, ket)
            print("L=%d parts=%s %s: got %r want %r bound %.3e" % (L, parts, ops, g, want, _bound(bra, ket)))
            assert abs(g - want) <= _bound(bra, ket), ops
            v, p = mp.chain(ops, L, parts, ket)
            if v is None or p != parts:
                assert g == 0, ops  # no sector, or another sector: exactly 0
            nonzero += want != 0
        assert nonzero >= (4 if min(parts) > 0 else 1)
        got = e.many_point_of(MEASURES, L, parts[0], parts[1], bra, ket, convention="measure")
        for vops, g in zip(MEASURES, got):
            assert abs(g - mp.measure(vops, L, parts, bra, ket)) <= _bound(bra, ket), vops


# ---- the L = 10 ring's two lowest states: 63504 states, 32 kernel tiles, several workgroups in the reduction ------------------------------------------
RING10 = [
    [("n", 0, UP)], [("n", 3, DOWN)], [("c", 2, UP), ("cdagger", 5, UP)], [("c", 9, DOWN), ("cdagger", 0, DOWN)],
    [("c", 1, UP), ("c", 1, DOWN), ("cdagger", 6, DOWN), ("cdagger", 6, UP)],  # on-site pair hopping
    [("c", 1, UP), ("c", 2, DOWN), ("cdagger", 8, DOWN), ("cdagger", 7, UP)],
    [("n", 0, UP), ("n", 4, DOWN), ("n", 9, UP)], [("sz", 0, UP), ("sz", 5, UP)], [("sz", 2, UP), ("sz", 3, UP), ("sz", 9, UP)],
    [("splus", 4, UP), ("sminus", 7, UP)], [("sminus", 0, UP), ("sz", 0, UP), ("splus", 9, UP)],
    [("c", 0, UP), ("n", 1, UP), ("cdagger", 2, DOWN)],  # another sector: 0
    [("sz", 1, UP), ("c", 1, UP), ("sz", 1, UP), ("cdagger", 1, UP)], [("n", 5, DOWN)], [("c", 3, UP), ("cdagger", 3, UP)],
    [("cdagger", 3, UP), ("c", 3, UP)], [("c", 0, DOWN), ("c", 9, UP), ("cdagger", 9, UP), ("cdagger", 0, DOWN)], [("n", 9, UP), ("n", 9, DOWN)],
    [("c", 4, UP), ("c", 5, DOWN), ("cdagger", 4, DOWN), ("cdagger", 5, UP)],
]
assert len(RING10) == 19  # more than two launches of 8: forces the host to split


@pytest.fixture(scope="module")
def ring10():
    L, nup, ndown = 10, 5, 5
    e = LanczosEngine()
    e.assemble_hubbard(L, nup, ndown, _ring(L), np.full(L, 4.0))
    e.keep_states(2)
    e.lanczos(2, want_vectors=False)
    psi = [e.state(0), e.state(1)]
    want = {(b, k): [mp.many_point(ops, L, (nup, ndown), psi[b], psi[k]) for ops in RING10] for b, k in ((0, 0), (0, 1))}  # computed once, shared
    yield e, L, (nup, ndown), psi, want
    e.close()


def test_many_point_kept_states(ring10):
    e, L, parts, psi, want = ring10
    for b, k in ((0, 0), (0, 1)):
        got = e.many_point(RING10, bra=b, ket=k)
        bound = _bound(psi[b], psi[k])
        for ops, g, w in zip(RING10, got, want[(b, k)]):
            print("bra %d ket %d %s: got %.17g want %.17g bound %.3e" % (b, k, ops, g, w, bound))
            assert abs(g - w) <= bound, ops
    assert abs(want[(0, 0)][4]) > 1e6 * _bound(psi[0], psi[0])  # the pair correlation is no trivial zero: the bound above resolves it to six digits
    text = e.many_point(["c?2?0;cdagger?5?0", "n?0?0;n?4?1;n?9?0"])
    assert text[0] == e.many_point([RING10[2]])[0] and text[1] == e.many_point([RING10[6]])[0]


# ---- 3. batching --------------------------------------------------------------------------------------------------------------------------------
def test_batches_are_bit_identical(ring10):
    e, L, parts, psi, want = ring10
    bits = lambda v: np.asarray(v, np.float64).view(np.uint64)  # noqa: E731
    all19 = e.many_point(RING10, bra=0, ket=1)
    again = e.many_point(RING10, bra=0, ket=1)
    assert np.array_equal(bits(all19), bits(again))  # fixed-order reduction
    first8 = e.many_point(RING10[:8], bra=0, ket=1)
    assert np.array_equal(bits(first8), bits(all19[:8]))
    singles = np.array([e.many_point([ops], bra=0, ket=1)[0] for ops in RING10])
    assert np.array_equal(bits(singles), bits(all19))
    shuffled = e.many_point(RING10[::-1], bra=0, ket=1)  # other slots, other neighbours
    assert np.array_equal(bits(shuffled[::-1]), bits(all19))


# ---- 4. physics pins on the ground state ----------------------------------------------------------------------------------------------------------
def test_physics_pins(ring10):
    e, L, (nup, ndown), psi, want = ring10
    for spin, count in ((UP, nup), (DOWN, ndown)):
        dens = e.many_point([[("n", i, spin)] for i in range(L)])
        nn, _ = e.two_point("n", (spin, spin))
        assert np.max(np.abs(dens - np.diag(nn))) <= 1e-12  # <n_i n_i> = <n_i>
        assert abs(np.sum(dens) - count) <= 1e-12
    # result[i, j] of two_point("c") = (c_j bra) . (c_i ket) = <bra| cdagger_j c_i |ket>: c_i listed first, it acts first
    cc, _ = e.two_point("c", (UP, UP))
    pairs = [(0, 0), (0, 1), (3, 7), (9, 2)]
    got = e.many_point([[("c", i, UP), ("cdagger", j, UP)] for i, j in pairs])
    for (i, j), g in zip(pairs, got):
        assert abs(g - cc[i, j]) <= 1e-12, (i, j)
    total = sum(e.measure([("c", i, UP, True), ("c", i, UP, False)]) for i in range(L))  # cdagger_i c_i, the LAST listed acts first
    assert abs(total - nup) <= 1e-12
    assert abs(e.measure([("sz", 2, UP, False)]) - (0.5 - dens_of(e, 2, UP))) <= 1e-12  # +1/2 empty, -1/2 occupied: 1/2 - <n>


def dens_of(e, site, spin):
    return e.many_point([[("n", site, spin)]])[0]


# ---- 5. zeros and refusals --------------------------------------------------------------------------------------------------------------------------
def test_zeros_and_refusals(ring10):
    e, L, parts, psi, want = ring10
    zeros = e.many_point([[("c", 0, UP)], [("c", 0, UP), ("n", 1, UP), ("cdagger", 2, DOWN)], [("splus", 1, UP)]])
    assert np.all(zeros == 0)  # final parts differ from the initial ones
    with LanczosEngine() as small:  # missing sectors: (0,0) on the way, a species beyond L
        v = oracle.fill_random(4, 3)
        assert np.all(small.many_point_of([[("c", 0, UP), ("cdagger", 0, UP)]], 4, 1, 0, v, v) == 0)
        v = oracle.fill_random(6, 3)
        assert np.all(small.many_point_of([[("cdagger", 0, UP), ("c", 0, UP)]], 4, 4, 2, v, v) == 0)
    with pytest.raises(LppError) as ei:
        e.measure([("c", 0, UP, False)])  # number changing
    assert ei.value.status == 1 and "conserve" in str(ei.value)
    with pytest.raises(LppError):
        e.many_point([[("n", L, UP)]])  # site >= L
    with pytest.raises(LppError):
        e.many_point([[("n", 0, UP)] * 17])
    with pytest.raises(ValueError):
        e.many_point([[("nn", 0, UP)]])
    with pytest.raises(LppError):
        e.many_point([[("n", 0, UP)]], bra=2)  # no such resident state
    hop = _ring(6)
    j = 0.5 * np.abs(hop)
    with LanczosEngine() as tj:
        tj.assemble_tj(6, 2, 2, hop, j, j, np.zeros((6, 6)))
        for call in (lambda: tj.many_point([[("n", 0, UP)]]), lambda: tj.measure([("n", 0, UP, False)]),
                     lambda: tj.apply_operator_string([("n", 0, UP)], 6, 2, 2, np.zeros(225))):
            with pytest.raises(LppError) as ei:
                call()
            assert ei.value.status == 1 and "t-J" in str(ei.value)
    with LanczosEngine() as hs:
        hs.assemble_heisenberg(6, 3, chain(6, 1.0, True), chain(6, 1.0, True))
        with pytest.raises(LppError) as ei:
            hs.many_point([[("sz", 0, UP)]])
        assert ei.value.status == 1 and "Heisenberg" in str(ei.value)


# ---- 6. the driver ------------------------------------------------------------------------------------------------------------------------------------
def test_driver_many_point_and_measure():
    """lanczos -f tests/golden/hubbard_ladder_2x4.inp -M ... -m ...: the printed values against the Python path on the same model and start vector.
    Both sides solve with the same kernels from the same start vector; -p 14 prints 14 digits and the comparison is held to 1e-8 absolute on values of
    order 0.1, the bound tests/test_gpu_observables.py holds the driver's two-point matrix to."""
    assert os.path.exists(DRIVER), "run __graft_entry__.build()"
    path = os.path.join(GOLD, "hubbard_ladder_2x4.inp")
    res = subprocess.run([DRIVER, "-f", path, "-p", "14", "-M", "n?0?0;n?1?1,c?0?0;cdagger?2?0", "-m", "<gs|n?0[0];n?1[1]|gs>"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    vals = {}
    for ln in lines:
        if ln.startswith("<gs|") and "|gs>=" in ln:
            vals[ln[:ln.index("|gs>=") + 4]] = float(ln.split("|gs>=")[1])
        elif ln.startswith("<gs|") and "|gs> = " in ln:
            vals["m:" + ln[:ln.index("|gs> = ") + 4]] = float(ln.split("|gs> = ")[1])
    assert set(vals) == {"<gs|n?0?0;n?1?1|gs>", "<gs|c?0?0;cdagger?2?0|gs>", "m:<gs|n?0[0];n?1[1]|gs>"}, lines
    inp = geometry.parse_input(open(path).read())
    L, nup, ndown = int(inp["TotalNumberOfSites"]), int(inp["TargetElectronsUp"]), int(inp["TargetElectronsDown"])
    with LanczosEngine() as e:
        e.assemble_hubbard(L, nup, ndown, geometry.terms_from_input(inp)[0], inp["hubbardU"], inp["potentialV"])
        e.keep_states(1)
        e.lanczos(1, init=oracle.fill_random(e.rows(), 1234), want_vectors=False)
        want = e.many_point(["n?0?0;n?1?1", "c?0?0;cdagger?2?0"])
        wm = e.measure([("n", 0, UP, False), ("n", 1, DOWN, False)])
    print("driver: %r against %r, %r" % (vals, want, wm))
    assert abs(vals["<gs|n?0?0;n?1?1|gs>"] - want[0]) <= 1e-8 and abs(vals["<gs|c?0?0;cdagger?2?0|gs>"] - want[1]) <= 1e-8
    assert abs(vals["m:<gs|n?0[0];n?1[1]|gs>"] - wm) <= 1e-8 and abs(wm - want[0]) <= 1e-12
    assert 0 < want[0] < 1 and abs(want[1]) > 1e-3
    # a t-J input is refused by the model's name
    bad = subprocess.run([DRIVER, "-f", os.path.join(GOLD, "tj_chain_L8_complex.inp"), "-M", "n?0?0"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "LPP_ERR_INVALID" in bad.stderr and "TjMultiOrb" in bad.stderr, bad.stderr
