"""Operator strings of the S = 1/2 Heisenberg basis on the GPU (basis="spin_half"): the string applied to a vector element by element, brackets of random
vectors, brackets of resident states with their batching and bit identity, pins against two_point, the refusals and `lanczos -M` on a Heisenberg
input -- against tests/heis_many_point_reference.py, a chain of accModifiedState_ steps on the word list that knows neither masks nor runs."""
import os
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import heis_many_point_reference as mp
import heis_obs_reference as ref
import oracle
from heis_many_point_reference import DOWN, UP
from helpers import chain
from lanczosplusplus_amd import LanczosEngine, LppError, geometry, operator_string_plan_heis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "lanczosplusplus_amd", "host", "lanczos")
GOLD = os.path.join(ROOT, "tests", "golden")
NAME = "heisenberg_chain_L12.inp"

pytestmark = pytest.mark.gpu

# (7;2): 21 states, an odd length with a half-unit tail, one run.  (14;7): 3432 states, the smallest with a high part.  (16;7): 11440 states, several
# tiles.  (18;9): 48620 states in 64 runs.
SECTORS = [(7, 2), (14, 7), (16, 7), (18, 9)]
SIZES = {7: 21, 14: 3432, 16: 11440, 18: 48620}


@lru_cache(maxsize=None)
def _chains(L, m, cplx):
    """(ket, [(string ket, final szPlusConst) for the 13 strings]) of the reference, computed once per sector and dtype"""
    ket = oracle.fill_random(ref.size(L, m), 11, cplx)
    ket.setflags(write=False)
    return ket, [mp.apply_string(s, L, m, ket) for s in mp.strings(L)]


# ---- 1. the string applied to a vector ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("L,m", SECTORS)
def test_apply_operator_string_heis(dtype, L, m):
    """every string against the reference chain: each output element is one product, so 1e-14 of the largest as in test_apply_operator_heis"""
    cplx = dtype == "c128"
    src, chains = _chains(L, m, cplx)
    assert len(src) == SIZES[L]
    factor = (0.75 - 0.5j) if cplx else -1.25
    nonzero = 0
    with LanczosEngine(dtype=dtype) as e:
        for k, string in enumerate(mp.strings(L)):
            unit, new = chains[k]
            want = factor * unit
            z, parts = e.apply_operator_string(string, L, m, 0, src, factor=factor, basis="spin_half")
            assert parts == (new, 0) and len(z) == ref.size(L, new) and z.dtype == src.dtype, k
            scale = np.max(np.abs(want))
            if k in mp.DEAD:
                assert scale == 0 and not z.any(), k
                continue
            assert scale > 0, k
            nonzero += new == m
            print("apply string %d (%d;%d) %s: max deviation %.3e of %.3e" % (k, L, m, dtype, np.max(np.abs(z - want)), scale))
            assert np.max(np.abs(z - want)) <= 1e-14 * scale, k
            assert np.all(z[unit == 0] == 0), k  # untouched destinations
            z2, _ = e.apply_operator_string(string, L, m, 0, src, factor=factor, out=z, basis="spin_half")
            assert np.max(np.abs(z2 - 2 * want)) <= 2e-14 * scale and np.all(z2[unit == 0] == 0), k
        assert nonzero >= 10
        # a dead string on top of a vector leaves it as it is
        keep = oracle.fill_random(ref.size(L, m), 3, cplx)
        z, _ = e.apply_operator_string(mp.strings(L)[9], L, m, 0, src, out=keep.copy(), basis="spin_half")
        assert np.array_equal(z, keep)


def test_apply_operator_string_heis_long_chain():
    """40 sites, three up spins (9880 states): the cut of the word is at 14 bits -- the largest LDS tables, 64 KiB -- and most runs hold one element.
    With factor 1 the result is the expanded plan exactly (tests/test_heis_many_point_host.py checks that against a direct enumeration)."""
    L, m = 40, 3
    src = oracle.fill_random(9880, 5)
    bra = oracle.fill_random(9880, 6)
    strings = ([("sminus", 0, UP), ("splus", 39, UP)], [("sz", 13, UP), ("sz", 14, UP)], [("sminus", 13, UP), ("splus", 14, UP)], [("sminus", 39, UP)],
               [("sz", 20, UP), ("n", 30, DOWN)])
    with LanczosEngine() as e:
        for string in strings:
            plan = operator_string_plan_heis(string, L, m)
            assert plan["lb"] == 14
            a = plan["action"]
            want = np.where(a != 0, np.sign(a) * src[np.maximum(np.abs(a) - 1, 0)], 0.0)
            z, parts = e.apply_operator_string(string, L, m, 0, src, basis="spin_half")
            assert parts == (plan["szPlusConst"], 0) and len(z) == len(a) and np.any(want != 0)
            assert np.array_equal(z, want), string
        # the bracket kernel with the same tables
        keep = [s for s in strings if operator_string_plan_heis(s, L, m, action=False)["szPlusConst"] == m]
        got = e.many_point_of(keep, L, m, 0, bra, src, basis="spin_half")
        for g, s in zip(got, keep):
            a = operator_string_plan_heis(s, L, m)["action"]
            want = np.dot(bra, np.where(a != 0, np.sign(a) * src[np.maximum(np.abs(a) - 1, 0)], 0.0))
            assert want != 0 and abs(g - want) <= _bound(bra, src), s


# ---- 2. brackets of random vectors --------------------------------------------------------------------------------------------------------------
def _bound(bra, ket):
    """the bound of tests/test_gpu_many_point.py: a dot product of n terms in any order with Cauchy-Schwarz, n 2^-53 |bra| |ket|.  One wrong sign or
    index moves the sum by about 1/n of the norm product, far above it."""
    return len(bra) * 2.0 ** -53 * np.linalg.norm(bra) * np.linalg.norm(ket)


@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("L,m", SECTORS)
def test_many_point_random_vectors(dtype, L, m):
    cplx = dtype == "c128"
    ket, chains = _chains(L, m, cplx)
    bra = oracle.fill_random(len(ket), 12, cplx)
    strings = mp.strings(L)
    with LanczosEngine(dtype=dtype) as e:
        got = e.many_point_of(strings, L, m, 0, bra, ket, basis="spin_half")
    assert len(got) == 13 and got.dtype == ket.dtype
    nonzero = 0
    for k, (vec, new) in enumerate(chains):
        if k in mp.DEAD or k in mp.LEAVES:
            assert got[k] == 0, k
            continue
        want = np.vdot(bra, vec)
        assert new == m
        print("bracket %d (%d;%d) %s: deviation %.3e, bound %.3e, value %.6e" % (k, L, m, dtype, abs(got[k] - want), _bound(bra, ket), abs(want)))
        assert abs(got[k] - want) <= _bound(bra, ket), k
        nonzero += abs(got[k]) > 100 * _bound(bra, ket)
    assert nonzero >= 10


# ---- 3. resident states: batches, text strings, bit identity; pins against two_point ---------------------------------------------------------------
def _ring16():
    """the ring of tests/test_gpu_heis_observables.py: (16;8), 12870 states, a site-dependent field"""
    L, m = 16, 8
    return L, m, chain(L, 1.0, True), chain(L, 0.7, True), np.linspace(-0.3, 0.4, L)


@pytest.fixture(scope="module")
def ring16():
    L, m, jpm, jzz, h = _ring16()
    with LanczosEngine(reortho=True, max_steps=150, eps=1e-11) as e:
        e.assemble_heisenberg(L, m, jpm, jzz, h)
        e.keep_states(2)
        e.lanczos(2, want_vectors=False)
        yield e, L, m, e.state(0), e.state(1)


def _many(L):
    """the 13 strings and 8 more: 21 strings, 18 of which are launched -- three batches"""
    return mp.strings(L) + [[("sz", i, UP), ("sz", (i + 5) % L, UP)] for i in range(4)] + [[("splus", i, UP), ("sminus", L - 1 - i, UP)] for i in range(4)]


def test_many_point_resident_states(ring16):
    e, L, m, gs, ex = ring16
    assert len(gs) == 12870
    strings = _many(L)
    assert len(strings) >= 19
    for bra, ket, bv, kv in ((0, 0, gs, gs), (0, 1, gs, ex)):
        got = e.many_point(strings, bra=bra, ket=ket, basis="spin_half")
        nonzero = 0
        for k, s in enumerate(strings):
            want = mp.many_point(s, L, m, bv, kv)
            assert abs(got[k] - want) <= _bound(bv, kv), (k, bra, ket)
            if k in mp.DEAD or k in mp.LEAVES:
                assert got[k] == 0
            # (between two orthogonal states a value may be small; that it is not the exact 0 of a string never launched is what counts there)
            nonzero += (abs(got[k]) > 100 * _bound(bv, kv)) if bra == ket else (got[k] != 0)
        assert nonzero >= 10
    # text strings are the same strings
    tuples = e.many_point(strings, basis="spin_half")
    texts = e.many_point([mp.text(s) for s in strings], basis="spin_half")
    assert np.array_equal(tuples.view(np.uint64), texts.view(np.uint64))


def test_many_point_bit_identity(ring16):
    """a value does not depend on the batch it is computed in, nor on the call"""
    e, L, m, _, _ = ring16
    strings = _many(L)[:19]
    every = e.many_point(strings, bra=0, ket=1, basis="spin_half").view(np.uint64)
    assert np.count_nonzero(every) >= 10
    assert np.array_equal(e.many_point(strings, bra=0, ket=1, basis="spin_half").view(np.uint64), every)
    assert np.array_equal(e.many_point(strings[:8], bra=0, ket=1, basis="spin_half").view(np.uint64), every[:8])
    assert np.array_equal(e.many_point(strings[::-1], bra=0, ket=1, basis="spin_half").view(np.uint64), every[::-1])
    for k, s in enumerate(strings):
        assert e.many_point([s], bra=0, ket=1, basis="spin_half").view(np.uint64)[0] == every[k], k


def test_many_point_against_two_point(ring16):
    """algebraic identities on the ground state.  two_point builds sz as n_up/2 - n_down/2 = bit - 1/2 and the string's sz is 1 - 2 bit, so the product
    of two is 4 times the former; splus i, sminus j is <gs| S-_j S+_i |gs>, which two_point("splus") has at [i, j].  Tolerances as argued in
    test_two_point_heis: normalised states, 12870 terms, far below 1e-12 per entry (times 4 for sz)."""
    e, L, m, _, _ = ring16
    pairs = [(0, 0), (0, 1), (3, 13), (15, 2)]
    zz, _ = e.two_point("sz", (0, 0))
    pm, _ = e.two_point("splus", (0, 0))
    got_zz = e.many_point([[("sz", i, UP), ("sz", j, UP)] for i, j in pairs], basis="spin_half")
    got_pm = e.many_point([[("splus", i, UP), ("sminus", j, UP)] for i, j in pairs], basis="spin_half")
    for k, (i, j) in enumerate(pairs):
        print("pins (%d,%d): sz %.3e splus %.3e" % (i, j, abs(got_zz[k] - 4 * zz[i, j]), abs(got_pm[k] - pm[i, j])))
        assert abs(got_zz[k] - 4 * zz[i, j]) <= 4e-12, (i, j)
        assert abs(got_pm[k] - pm[i, j]) <= 1e-12, (i, j)
    assert np.max(np.abs(got_zz)) > 0.1 and np.max(np.abs(got_pm)) > 0.1
    nup = e.many_point([[("n", i, UP)] for i in range(L)], basis="spin_half")
    assert abs(np.sum(nup) - m) <= 1e-10
    ndn = e.many_point([[("n", i, DOWN)] for i in range(L)], basis="spin_half")
    assert abs(np.sum(ndn) - (L - m)) <= 1e-10


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ring16):
    e, L, m, gs, _ = ring16
    with pytest.raises(LppError) as ei:
        e.many_point([[("sz", 0, UP)]])  # the opt-in is explicit
    assert ei.value.status == 1 and "Heisenberg" in str(ei.value) and "spin_half" in str(ei.value)
    with pytest.raises(LppError) as ei:
        e.measure([("sz", 0, UP, False)])
    assert ei.value.status == 1 and "Heisenberg" in str(ei.value)
    for bad in ([("c", 0, UP)], [("sz", 0, UP), ("cdagger", 1, UP)], [("sz", L, UP)], [("sz", 0, UP)] * 17, []):
        with pytest.raises(LppError) as ei:
            e.many_point([bad], basis="spin_half")
        assert ei.value.status == 1, bad
    with pytest.raises(LppError):
        e.many_point([[("sz", 0, UP)]], bra=2, basis="spin_half")  # no such resident state
    with pytest.raises((ValueError, LppError)):
        e.many_point([[("sz", 0, UP, False)]], convention="measure", basis="spin_half")
    with pytest.raises((ValueError, LppError)):
        e.many_point_of([[("sz", 0, UP, False)]], L, m, 0, gs, gs, convention="measure", basis="spin_half")
    with pytest.raises((ValueError, LppError)):
        e.apply_operator_string([("sz", 0, UP, False)], L, m, 0, gs, convention="measure", basis="spin_half")
    with pytest.raises(ValueError):
        e.many_point([[("sz", 0, UP)]], basis="tj")
    with pytest.raises(LppError) as ei:  # without the opt-in the host-vector forms refuse a Heisenberg engine too
        e.many_point_of([[("n", 0, UP)]], L, m, 0, gs, gs)
    assert ei.value.status == 1 and "Heisenberg" in str(ei.value)
    # the sector walk: S+ met in the all-up sector, S- in the all-down one, at the step that meets it
    one = np.ones(1)
    with pytest.raises(LppError) as ei:
        e.many_point_of([[("splus", 0, UP)]], 4, 4, 0, one, one, basis="spin_half")
    assert ei.value.status == 1
    with pytest.raises(LppError) as ei:
        e.many_point_of([[("sminus", 0, UP), ("sminus", 1, UP)]], 4, 1, 0, np.ones(4), np.ones(4), basis="spin_half")
    assert ei.value.status == 1
    hop = chain(6, -1.0, True)
    with LanczosEngine() as hub:
        hub.assemble_hubbard(6, 3, 3, hop, np.full(6, 4.0))
        hub.keep_states(1)
        hub.lanczos(1, want_vectors=False)
        with pytest.raises(LppError) as ei:
            hub.many_point([[("sz", 0, UP)]], basis="spin_half")
        assert ei.value.status == 1
        assert hub.many_point([[("n", 0, UP)]])[0] > 0  # and its own strings are served as before
        # ... while the host-vector forms serve the spin basis on any engine that is not a t-J one
        v = oracle.fill_random(20, 2)
        assert abs(hub.many_point_of([[("sz", 0, UP), ("sz", 0, UP)]], 6, 3, 0, v, v, basis="spin_half")[0] - np.dot(v, v)) <= _bound(v, v)
    j = 0.5 * np.abs(hop)
    with LanczosEngine() as tj:
        tj.assemble_tj(6, 2, 2, hop, j, j, np.zeros((6, 6)))
        for call in (lambda: tj.many_point([[("n", 0, UP)]], basis="spin_half"), lambda: tj.many_point_of([[("n", 0, UP)]], 6, 3, 0, v, v, basis="spin_half"),
                     lambda: tj.apply_operator_string([("n", 0, UP)], 6, 3, 0, v, basis="spin_half")):
            with pytest.raises(LppError) as ei:
                call()
            assert ei.value.status == 1 and "t-J" in str(ei.value)
    with LanczosEngine() as big:  # twiceS = 2: the reference throws for higher spins
        big.assemble_heisenberg(6, 6, chain(6, 1.0, True), chain(6, 1.0, True), twiceS=2)
        big.keep_states(1)
        big.lanczos(1, want_vectors=False)
        with pytest.raises(LppError) as ei:
            big.many_point([[("sz", 0, UP)]], basis="spin_half")
        assert ei.value.status == 1


# ---- 5. the driver ------------------------------------------------------------------------------------------------------------------------------------
def test_driver_many_point_heis():
    """lanczos -f tests/golden/heisenberg_chain_L12.inp -M ...: the printed values against the Python path on the same model and start vector.  Both
    sides solve with the same kernels from the same start vector; -p 14 prints 14 digits and the comparison is held to 1e-8 absolute, the bound the
    other driver tests use."""
    assert os.path.exists(DRIVER), "run __graft_entry__.build()"
    path = os.path.join(GOLD, NAME)
    res = subprocess.run([DRIVER, "-f", path, "-p", "14", "-M", "sz?0?0;sz?5?0,splus?0?0;sminus?3?0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    vals = {}
    for ln in res.stdout.splitlines():
        if ln.startswith("<gs|") and "|gs>=" in ln:
            vals[ln[:ln.index("|gs>=") + 4]] = float(ln.split("|gs>=")[1])
    assert set(vals) == {"<gs|sz?0?0;sz?5?0|gs>", "<gs|splus?0?0;sminus?3?0|gs>"}, res.stdout
    inp = geometry.parse_input(open(path).read())
    assert inp["Model"] == "Heisenberg" and int(inp["HeisenbergTwiceS"]) == 1
    terms = geometry.terms_from_input(inp)
    with LanczosEngine() as e:
        e.assemble_heisenberg(int(inp["TotalNumberOfSites"]), int(inp["TargetSzPlusConst"]), terms[0], terms[1], np.asarray(inp["MagneticField"], np.float64))
        e.keep_states(1)
        e.lanczos(1, init=oracle.fill_random(e.rows(), 1234), want_vectors=False)
        want = e.many_point(["sz?0?0;sz?5?0", "splus?0?0;sminus?3?0"], basis="spin_half")
    print("driver Heisenberg -M: %s against %s" % (vals, want))
    assert abs(vals["<gs|sz?0?0;sz?5?0|gs>"] - want[0]) <= 1e-8 and abs(vals["<gs|splus?0?0;sminus?3?0|gs>"] - want[1]) <= 1e-8
    assert abs(want[0]) > 1e-3 and abs(want[1]) > 1e-3
    # -m stays refused on a Heisenberg input
    bad = subprocess.run([DRIVER, "-f", path, "-m", "<gs|sz[0]|gs>"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "Heisenberg" in bad.stderr + bad.stdout
