"""Operator strings of the one-orbital t-J basis on the GPU (basis="tj"): the string applied to a vector element by element, brackets of random vectors,
brackets of resident states on the general layout and on a hole-major engine with their batching and bit identity, pins against two_point, and
`lanczos -M` on a t-J input that opts in -- against tests/tj_many_point_reference.py, a chain of accModifiedState_ steps on the sorted word list that
knows neither patterns nor masks nor tables."""
import os
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import oracle
import tj_many_point_reference as mp
import tj_obs_reference as ref
from helpers import chain
from lanczosplusplus_amd import LanczosEngine, LppError, geometry, operator_string_plan_tj
from tj_many_point_reference import DOWN, UP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "lanczosplusplus_amd", "host", "lanczos")
GOLD = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

# (7;1,2): 105 states, an odd length with the half-unit tail, blocks of 5.  (7;2,2): 210.  (10;3,3): 4200 states, three tiles.  (12;4,4): 34650.
SECTORS = [(7, 1, 2), (7, 2, 2), (10, 3, 3), (12, 4, 4)]
SIZES = {(7, 1, 2): 105, (7, 2, 2): 210, (10, 3, 3): 4200, (12, 4, 4): 34650}
STAYING = {(7, 1, 2): 10, (7, 2, 2): 11, (10, 3, 3): 11, (12, 4, 4): 11}  # non-zero strings that stay (worked out on the restatement)


@lru_cache(maxsize=None)
def _chains(L, nup, ndown, cplx):
    """(ket, [(string ket, final parts) or (None, None) for the 15 strings]) of the reference, computed once per sector and dtype"""
    ket = oracle.fill_random(ref.size(L, nup, ndown), 11, cplx)
    ket.setflags(write=False)
    return ket, [mp.apply_string(s, L, (nup, ndown), ket) for s in mp.strings(L)]


def _bound(bra, ket):
    """the bound of tests/test_gpu_many_point.py: a dot product of n terms in any order with Cauchy-Schwarz, n 2^-53 |bra| |ket|"""
    return len(bra) * 2.0 ** -53 * np.linalg.norm(bra) * np.linalg.norm(ket)


def _applied(a, src):
    """an expanded plan applied to src"""
    return np.where(a != 0, np.sign(a) * src[np.maximum(np.abs(a) - 1, 0)], 0.0)


# ---- 1. the string applied to a vector ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("L,nup,ndown", SECTORS)
def test_apply_operator_string_tj(dtype, L, nup, ndown):
    """every string against the reference chain: each output element is one product, so 1e-14 of the largest as in test_apply_operator_string_heis"""
    cplx = dtype == "c128"
    parts = (nup, ndown)
    src, chains = _chains(L, nup, ndown, cplx)
    assert len(src) == SIZES[(L,) + parts]
    factor = (0.75 - 0.5j) if cplx else -1.25
    nonzero, dead = 0, None
    with LanczosEngine(dtype=dtype) as e:
        for k, string in enumerate(mp.strings(L)):
            unit, new = chains[k]
            z, got_parts = e.apply_operator_string(string, L, nup, ndown, src, factor=factor, basis="tj")
            if unit is None:
                assert (z, got_parts) == (None, None), k
                continue
            want = factor * unit
            assert got_parts == new and len(z) == ref.size(L, *new) and z.dtype == src.dtype, k
            scale = np.max(np.abs(want))
            plan = operator_string_plan_tj(string, L, nup, ndown)
            if plan["dead"]:
                assert scale == 0 and not z.any(), k
                dead = string
                continue
            print("apply string %d (%d;%d,%d) %s: max deviation %.3e of %.3e" % (k, L, nup, ndown, dtype, np.max(np.abs(z - want)), scale))
            assert np.max(np.abs(z - want)) <= 1e-14 * scale, k
            assert np.all(z[unit == 0] == 0), k  # untouched destinations
            nonzero += scale > 0 and new == parts
            z2, _ = e.apply_operator_string(string, L, nup, ndown, src, factor=factor, out=z, basis="tj")
            assert np.max(np.abs(z2 - 2 * want)) <= 2e-14 * scale and np.all(z2[unit == 0] == 0), k
            # with factor 1 the result is the expanded plan applied to src, exactly
            z1, _ = e.apply_operator_string(string, L, nup, ndown, src, basis="tj")
            assert np.array_equal(z1, _applied(plan["action"], src)), k
        assert nonzero >= STAYING[(L,) + parts]
        # a dead string on top of a vector leaves it as it is
        assert dead is not None
        plan =operator_string_plan_tj(dead, L, nup, ndown, action=False)
        keep = oracle.fill_random(plan["n_dst"], 3, cplx)
        z, _ = e.apply_operator_string(dead, L, nup, ndown, src, out=keep.copy(), basis="tj")
        assert np.array_equal(z, keep)


# ---- 2. edges: one block, blocks of one element, the full lattice ------------------------------------------------------------------------------------
EDGES = [(8, 3, 0, [[("c", 0, UP), ("cdagger", 5, UP)], [("n", 2, UP)], [("sminus", 1, UP), ("splus", 1, UP)], [("n", 2, DOWN)], [("sminus", 0, UP)]]),
         (9, 0, 3, [[("c", 0, DOWN), ("cdagger", 5, DOWN)], [("n", 2, DOWN)], [("splus", 4, UP), ("sminus", 4, UP)], [("splus", 0, UP), ("sminus", 8, UP)], [("splus", 3, UP)]]),
         (6, 3, 3, [[("cdagger", 0, UP)], [("c", 1, UP), ("cdagger", 1, UP)], [("splus", 0, UP), ("sminus", 5, UP)], [("c", 2, DOWN), ("cdagger", 2, UP)], [("n", 4, DOWN)]])]


@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("L,nup,ndown,strings", EDGES)
def test_edges(dtype, L, nup, ndown, strings):
    cplx = dtype == "c128"
    parts = (nup, ndown)
    src = oracle.fill_random(ref.size(L, *parts), 7, cplx)
    bra = oracle.fill_random(len(src), 8, cplx)
    live = 0
    with LanczosEngine(dtype=dtype) as e:
        for string in strings:
            unit, new = mp.apply_string(string, L, parts, src)
            z, got = e.apply_operator_string(string, L, nup, ndown, src, basis="tj")
            if unit is None:
                assert (z, got) == (None, None), string
            else:
                assert got == new and np.array_equal(z, unit), string  # (factor 1: every element is a copy or its negative)
                live += bool(unit.any())
        got = e.many_point_of(strings, L, nup, ndown, bra, src, basis="tj")
        for g, string in zip(got, strings):
            want = mp.many_point(string, L, parts, bra, src)
            assert abs(g - want) <= _bound(bra, src), string
            if want == 0:
                assert g == 0, string
    assert live >= 3


# ---- 3. brackets of random vectors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("L,nup,ndown", SECTORS)
def test_many_point_random_vectors(dtype, L, nup, ndown):
    cplx = dtype == "c128"
    parts = (nup, ndown)
    ket, chains = _chains(L, nup, ndown, cplx)
    bra = oracle.fill_random(len(ket), 12, cplx)
    strings = mp.strings(L)
    with LanczosEngine(dtype=dtype) as e:
        got = e.many_point_of(strings, L, nup, ndown, bra, ket, basis="tj")
    assert len(got) == 15 and got.dtype == ket.dtype
    nonzero = 0
    for k, (vec, new) in enumerate(chains):
        if vec is None or new != parts or not vec.any():
            assert got[k] == 0, k  # no sector, leaving, dead (or reaching nothing): never launched, or an exact zero
            continue
        want = np.vdot(bra, vec)
        print("bracket %d (%d;%d,%d) %s: deviation %.3e, bound %.3e, value %.6e" % (k, L, nup, ndown, dtype, abs(got[k] - want), _bound(bra, ket), abs(want)))
        assert abs(got[k] - want) <= _bound(bra, ket), k
        nonzero += abs(got[k]) > 100 * _bound(bra, ket)
    assert nonzero >= STAYING[(L,) + parts]


# ---- 4. resident states: both layouts, batches, text strings, bit identity; pins against two_point -------------------------------------------------
def _tj_ring(L):
    hop = chain(L, -1.0, True)
    j = 0.5 * np.abs(hop)
    return hop, j, j, np.zeros((L, L))


def _many(L):
    """the 15 strings and 6 more: 21 strings, at least 17 of which are launched -- three batches"""
    return mp.strings(L) + [[("n", i, UP), ("n", (i + 5) % L, DOWN)] for i in range(3)] + [[("splus", i, UP), ("sminus", L - 1 - i, UP)] for i in range(3)]


@pytest.fixture(scope="module", params=["0", "1"])
def ring12(request):
    """a 12-site t-J ring (4,4), 34650 states, two resident states: the general layout, and the hole-major form (layout kernel 5)"""
    L, nup, ndown = 12, 4, 4
    mpatch = pytest.MonkeyPatch()
    mpatch.setenv("LPP_TJ_LAYOUT", request.param)
    try:
        with LanczosEngine(reortho=True, max_steps=150, eps=1e-11) as e:
            e.assemble_tj(L, nup, ndown, *_tj_ring(L))
            assert (e.layout()["kernel"] == 5) == (request.param == "1")
            e.keep_states_tj(2)
            e.lanczos(2, want_vectors=False)
            yield e, L, (nup, ndown), e.state(0), e.state(1)
    finally:
        mpatch.undo()


def test_many_point_resident_states(ring12):
    e, L, parts, gs, ex = ring12
    assert len(gs) == 34650
    strings = _many(L)
    assert len(strings) == 21
    launched = sum(1 for s in strings if (lambda p: p is not None and not p["dead"] and (p["nup"], p["ndown"]) == parts)(operator_string_plan_tj(s, L, *parts, action=False)))
    assert launched >= 17
    for bra, ket, bv, kv in ((0, 0, gs, gs), (0, 1, gs, ex)):
        got = e.many_point(strings, bra=bra, ket=ket, basis="tj")
        nonzero = 0
        for k, s in enumerate(strings):
            want = mp.many_point(s, L, parts, bv, kv)
            assert abs(got[k] - want) <= _bound(bv, kv), (k, bra, ket)
            if want == 0:
                assert got[k] == 0, k
            nonzero += (abs(got[k]) > 100 * _bound(bv, kv)) if bra == ket else (got[k] != 0)
        assert nonzero >= 11
    # text strings are the same strings
    tuples = e.many_point(strings, basis="tj")
    texts = e.many_point([mp.text(s) for s in strings], basis="tj")
    assert np.array_equal(tuples.view(np.uint64), texts.view(np.uint64))


def test_many_point_bit_identity(ring12):
    """a value does not depend on the batch it is computed in, nor on the call; sz is n of the given spin"""
    e, L, parts, _, _ = ring12
    strings = _many(L)[:19]
    every = e.many_point(strings, bra=0, ket=1, basis="tj").view(np.uint64)
    assert np.count_nonzero(every) >= 11
    assert np.array_equal(e.many_point(strings, bra=0, ket=1, basis="tj").view(np.uint64), every)
    assert np.array_equal(e.many_point(strings[:8], bra=0, ket=1, basis="tj").view(np.uint64), every[:8])
    assert np.array_equal(e.many_point(strings[::-1], bra=0, ket=1, basis="tj").view(np.uint64), every[::-1])
    for k, s in enumerate(strings):
        assert e.many_point([s], bra=0, ket=1, basis="tj").view(np.uint64)[0] == every[k], k
    for i, s in ((0, UP), (5, DOWN), (11, UP)):
        a = e.many_point([[("sz", i, s)], [("n", i, s)]], basis="tj").view(np.uint64)
        assert a[0] == a[1] and a[0] != 0


def test_many_point_against_two_point(ring12):
    """algebraic identities on the ground state: c i, cdagger j is <gs| cdagger_j c_i |gs>, which two_point("c") has at [i, j].  Normalised states,
    34650 terms: the argument of test_many_point_against_two_point, 1e-12 per entry"""
    e, L, (nup, ndown), _, _ = ring12
    pairs = [(0, 0), (0, 1), (3, 10), (11, 2)]
    for s in (UP, DOWN):
        cc, _ = e.two_point("c", (s, s))
        got = e.many_point([[("c", i, s), ("cdagger", j, s)] for i, j in pairs], basis="tj")
        for k, (i, j) in enumerate(pairs):
            print("pins spin %d (%d,%d): %.3e" % (s, i, j, abs(got[k] - cc[i, j])))
            assert abs(got[k] - cc[i, j]) <= 1e-12, (s, i, j)
        assert np.max(np.abs(got)) > 0.1
    n_up = e.many_point([[("n", i, UP)] for i in range(L)], basis="tj")
    assert abs(np.sum(n_up) - nup) <= 1e-10
    n_dn = e.many_point([[("n", i, DOWN)] for i in range(L)], basis="tj")
    assert abs(np.sum(n_dn) - ndown) <= 1e-10


# ---- 5. the Python layer's refusals ---------------------------------------------------------------------------------------------------------------
def test_python_refusals(ring12):
    e, L, (nup, ndown), gs, _ = ring12
    for call in (lambda: e.many_point([[("n", 0, UP)]]), lambda: e.measure([("n", 0, UP, False)]), lambda: e.many_point([[("n", 0, UP)]], basis="spin_half"),
                 lambda: e.many_point_of([[("n", 0, UP)]], L, nup, ndown, gs, gs)):
        with pytest.raises(LppError) as ei:
            call()
        assert ei.value.status == 1 and "t-J" in str(ei.value)
    with pytest.raises(ValueError):
        e.many_point([[("n", 0, UP, False)]], convention="measure", basis="tj")
    with pytest.raises(LppError) as ei:
        e.many_point([[("splus", 0, DOWN)]], basis="tj")
    assert ei.value.status == 1
    with pytest.raises(LppError):
        e.many_point([[("n", L, UP)]], basis="tj")
    with LanczosEngine() as hub:  # the host-vector forms need no matrix; many_point needs an engine set up by assemble_tj
        v = oracle.fill_random(105, 2)
        want = mp.many_point([("n", 0, UP), ("n", 6, DOWN)], 7, (1, 2), v, v)
        assert abs(hub.many_point_of([[("n", 0, UP), ("n", 6, DOWN)]], 7, 1, 2, v, v, basis="tj")[0] - want) <= _bound(v, v)
        with pytest.raises(ValueError):
            hub.many_point([[("n", 0, UP)]], basis="tj")


# ---- 6. the driver ------------------------------------------------------------------------------------------------------------------------------
def test_driver_many_point_tj():
    """lanczos -M on the L8 input that opts in with SolverOptions=useComplex,TjOperatorStrings against many_point(basis="tj") on the same model and start
    vector, within the 1e-8 of the other driver tests; -m stays refused"""
    assert os.path.exists(DRIVER), "run __graft_entry__.build()"
    name = os.path.join(GOLD, "tj_chain_L8_strings.inp")
    texts = ["n?0?0;n?7?1", "c?0?0;cdagger?3?0", "splus?1?0;sminus?4?0"]
    res = subprocess.run([DRIVER, "-f", name, "-p", "14", "-M", ",".join(texts)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    vals = {}
    for ln in res.stdout.splitlines():
        if ln.startswith("<gs|") and "|gs>=" in ln:
            key, val = ln.split("|gs>=")
            val = val.strip()
            vals[key[4:]] = complex(*[float(x) for x in val.strip("()").split(",")]) if val.startswith("(") else complex(float(val))
    inp = geometry.parse_input(open(name).read())
    L, nup, ndown = int(inp["TotalNumberOfSites"]), int(inp["TargetElectronsUp"]), int(inp["TargetElectronsDown"])
    with LanczosEngine(dtype="c128") as e:
        e.assemble_tj(L, nup, ndown, *tuple(geometry.terms_from_input(inp)[:4]), potentialV=inp.get("potentialV"))
        e.keep_states_tj(1)
        e.lanczos(1, init=oracle.fill_random(e.rows(), 1234, True), want_vectors=False)
        want = e.many_point(texts, basis="tj")
    print("driver t-J -M: %r against %r" % (vals, want))
    for t, w in zip(texts, want):
        assert abs(vals[t] - w) <= 1e-8, t
    assert abs(want[0]) > 1e-3 and abs(want[1]) > 1e-3 and abs(want[2]) > 1e-3
    bad = subprocess.run([DRIVER, "-f", name, "-m", "<gs|n?0[0]|gs>"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "LPP_ERR_INVALID" in bad.stderr and "TjMultiOrb" in bad.stderr, bad.stderr
