"""The ten operator-string entry points of the C ABI (apply_string, apply_string_host, many_point, many_point_host, bench_string_dot, each with its _heis
form), which one driver over two string families serves: every refusal's status and text pinned, called below the Python layer (which refuses most of
these first), and the batching of many_point_of at the boundaries of a launch of 8 strings with strings in the list that launch nothing."""
import ctypes as C

import numpy as np
import pytest

import heis_many_point_reference as hmp
import heis_obs_reference as href
import many_point_reference as mp
import oracle
from helpers import chain
from lanczosplusplus_amd import LanczosEngine

pytestmark = pytest.mark.gpu

UP, DOWN = 0, 1
OP = dict(c=1, sz=2, cdagger=3, n=4, splus=5, sminus=6)
KINDS = ("apply", "apply_host", "many_point", "many_point_host", "bench")
NAME = {
    "": dict(apply="lpp_engine_apply_string", apply_host="lpp_engine_apply_string_host", many_point="lpp_engine_many_point", many_point_host="lpp_engine_many_point_host",
             bench="lpp_engine_bench_string_dot"),
    "_heis": dict(apply="lpp_engine_apply_string_heis", apply_host="lpp_engine_apply_string_heis_host", many_point="lpp_engine_many_point_heis",
                  many_point_host="lpp_engine_many_point_heis_host", bench="lpp_engine_bench_string_dot_heis"),
}
# a call that is served: one operator on the resident sector.  Hubbard ring L = 4 (2,2), 36 states; Heisenberg chain L = 6, szPlusConst = 3, 20 states
VALID = {
    "": dict(conv=0, ops=[OP["n"]], sites=[0], spins=[UP], off=[0, 1], L=4, nup=2, ndown=2, n=36),
    "_heis": dict(conv=0, ops=[OP["sz"]], sites=[0], spins=[UP], off=[0, 1], L=6, nup=3, ndown=0, n=20),
}


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(e, family, kind, **changes):
    """(status, lpp_last_error()) of one entry point with the arguments of VALID[family] but for `changes`.  null=True: the result / has / ms pointer is
    NULL.  The device-vector apply gets no vectors: every row below is refused before they are read."""
    a = dict(VALID[family], bra_state=0, ket_state=0, warmup=0, iters=1, null=False)
    a.update(changes)
    ops, sites, spins = (np.array(a[k], np.int32) for k in ("ops", "sites", "spins"))
    flags, off = np.zeros_like(ops), np.array(a["off"], np.int64)
    fn = getattr(e._lib, NAME[family][kind])
    sector = (a["L"], a["nup"], a["ndown"])
    x, y = np.ones(a["n"]), np.ones(a["n"])
    if kind in ("apply", "apply_host"):
        has, n1, n2 = C.c_int32(), C.c_int32(), C.c_int32()
        host = kind == "apply_host"
        st = fn(e._h, a["conv"], a.get("nops", len(ops)), _p(ops), _p(sites), _p(spins), _p(flags), *sector, 1.0, 0.0, _p(x) if host else None, _p(y) if host else None, 0,
                None if a["null"] else C.byref(has), C.byref(n1), C.byref(n2))
    else:
        res = np.zeros((max(len(off) - 1, 1), 2))
        head = (e._h, a["conv"], a.get("nstrings", len(off) - 1), _p(off), _p(ops), _p(sites), _p(spins), _p(flags)) + sector
        if kind == "many_point":
            st = fn(*head, a["bra_state"], a["ket_state"], None if a["null"] else _p(res))
        elif kind == "many_point_host":
            st = fn(*head, _p(x), _p(y), None if a["null"] else _p(res))
        else:
            ms, by = C.c_double(), C.c_double()
            st = fn(*head, a["warmup"], a["iters"], None if a["null"] else C.byref(ms), C.byref(by))
    msg = e._lib.lpp_last_error()
    return st, (msg.decode() if msg else "")


# ---- the table: (family, kinds, changes to the valid call, status, text; "@" stands for the entry point's own name) ------------------------------------
LISTS = ("many_point", "many_point_host", "bench")
APPLY = ("apply", "apply_host")
PLANNER = {"": "operator string", "_heis": "Heisenberg operator string"}
BAD_SECTOR = {"": dict(nup=5), "_heis": dict(L=63)}
BAD_SECTOR_TEXT = {"": ": bad sites / sector", "_heis": ": bad sites / sector (szPlusConst <= sites <= 62)"}
OTHER_SECTOR = {"": dict(nup=1, ndown=1), "_heis": dict(nup=2)}
NOT_RESIDENT = {"": "@: (sites, nup, ndown) is not the sector of the resident states", "_heis": "@: (sites, szPlusConst) is not the sector of the resident states"}
TJ_TEXT = {"": "@: the t-J model (TjMultiOrb) is not supported, operator strings are built for the Hubbard product basis",
           "_heis": "@: the t-J model (TjMultiOrb) is not supported, its operator strings are not built yet"}
LEAVES = {"": (dict(ops=[OP["c"]]), "@: a string that leaves the sector launches nothing"),
          "_heis": (dict(ops=[OP["splus"]]), "@: a string that is identically zero or leaves the sector launches nothing")}
MEASURE_TEXT = "@: the Heisenberg basis has the many-point convention only (the labels of the measure convention are per fermion species)"
NINE = dict(ops=[OP["n"]] * 9, sites=[0] * 9, spins=[UP] * 9, off=list(range(10)))


def _rows():
    rows = []
    for f in ("", "_heis"):
        seventeen = dict(ops=VALID[f]["ops"] * 17, sites=[0] * 17, spins=[UP] * 17)
        rows += [
            # a null has / result pointer
            (f, APPLY + ("many_point", "many_point_host"), dict(null=True), 1, "@: null argument"),
            # a string of 0 and of 17 operators: the planner's words from apply, the list check's from the others; a negative offset is the same refusal
            (f, APPLY, dict(nops=0), 1, PLANNER[f] + ": 1 to 16 operators per string"),
            (f, APPLY, dict(nops=17, **seventeen), 1, PLANNER[f] + ": 1 to 16 operators per string"),
            (f, LISTS, dict(off=[0, 0]), 1, "@: 1 to 16 operators per string"),
            (f, LISTS, dict(off=[0, 17], **seventeen), 1, "@: 1 to 16 operators per string"),
            (f, LISTS, dict(off=[-1, 0]), 1, "@: 1 to 16 operators per string"),
            # a bad sector: nup > sites; for the Heisenberg basis 63 sites
            (f, APPLY, BAD_SECTOR[f], 1, PLANNER[f] + BAD_SECTOR_TEXT[f]),
            (f, LISTS, BAD_SECTOR[f], 1, "@" + BAD_SECTOR_TEXT[f]),
            # resident states: one that is not kept (LPP_ERR_STATE), a sector that is not theirs
            (f, ("many_point",), dict(bra_state=3), 5, "@: no such resident state (lpp_engine_keep_states before lpp_engine_lanczos)"),
            (f, ("many_point",), dict(ket_state=3), 5, "@: no such resident state (lpp_engine_keep_states before lpp_engine_lanczos)"),
            (f, ("many_point",), OTHER_SECTOR[f], 1, NOT_RESIDENT[f]),
            # the bench: one launch's strings, at least one timed step, strings that stay
            (f, ("bench",), dict(off=[0], nstrings=0), 1, "@: 1 to 8 strings (one launch)"),
            (f, ("bench",), NINE, 1, "@: 1 to 8 strings (one launch)"),
            (f, ("bench",), LEAVES[f][0], 1, LEAVES[f][1]),
            # what is served, so that a refusal above is the row's doing and not the harness's (the text of a served call is not compared)
            (f, ("apply_host", "many_point", "many_point_host", "bench"), dict(), 0, None),
        ]
    rows += [
        ("", ("bench",), dict(iters=0), 1, "@: bad argument"),
        # DELIBERATE CHANGE: ": null argument" before the string families shared one bench body; now as the Hubbard twin and bench_operator say
        ("_heis", ("bench",), dict(iters=0), 1, "@: bad argument"),
        ("", ("bench",), dict(NINE, **BAD_SECTOR[""]), 1, "@: 1 to 8 strings (one launch)"),
        # DELIBERATE CHANGE: the count and the sector both wrong -- the sector was reported first here and the count first by the Hubbard twin; now the count
        ("_heis", ("bench",), dict(NINE, **BAD_SECTOR["_heis"]), 1, "@: 1 to 8 strings (one launch)"),
        # the measure convention on each Heisenberg entry point
        ("_heis", KINDS, dict(conv=1), 1, MEASURE_TEXT),
    ]
    return rows


def _mismatches(e, rows, text_of=None):
    bad = []
    for family, kinds, changes, status, text in rows:
        for kind in kinds:
            st, msg = _call(e, family, kind, **changes)
            want = text_of[family] if text_of else text
            want = None if want is None else want.replace("@", NAME[family][kind])
            if st != status or (want is not None and msg != want):
                bad.append("%s %r: got (%d, %r), pinned (%d, %r)" % (NAME[family][kind], changes, st, msg, status, want))
    return bad


# What the C level knows of a t-J model is the hole-major form (lpp_tj.hip); the Python layer and the C++ shim refuse by the model's name.  An engine in
# that form is refused by all ten; the six-site one is too small for the form, so its strings are served like any engine's without resident states
SMALL_TJ = [(f, ("apply",), dict(), 1, "observables: null vector") for f in ("", "_heis")]
SMALL_TJ += [(f, ("many_point",), dict(), 5, "@: no such resident state (lpp_engine_keep_states before lpp_engine_lanczos)") for f in ("", "_heis")]
SMALL_TJ += [(f, ("apply_host", "many_point_host", "bench"), dict(), 0, None) for f in ("", "_heis")]


def test_string_entry_refusals_are_pinned(monkeypatch):
    """(status, text) of every refusal the ten entry points make before they launch, against the table above, in the order of the checks: null argument,
    the engine and the convention, the list, the count of a bench, the sector, the resident states.  The multi-rank refusal, one shared line, is not
    exercised."""
    bad = []
    hop = chain(6, -1.0, True)
    j = 0.5 * np.abs(hop)
    with LanczosEngine() as hub, LanczosEngine() as heis, LanczosEngine() as tj:
        hub.assemble_hubbard(4, 2, 2, chain(4, -1.0, True), np.full(4, 4.0))
        heis.assemble_heisenberg(6, 3, chain(6, 1.0), chain(6, 1.0))
        for e in (hub, heis):
            e.keep_states(1)
            e.lanczos(1, want_vectors=False)
        assert hub.rows() == 36 and heis.rows() == 20
        tj.assemble_tj(6, 2, 2, hop, j, j, np.zeros((6, 6)))
        rows = _rows()
        bad += _mismatches(hub, [r for r in rows if r[0] == ""])
        bad += _mismatches(heis, [r for r in rows if r[0] == "_heis"])
        bad += _mismatches(tj, SMALL_TJ)
    monkeypatch.setenv("LPP_TJ_LAYOUT", "1")  # below the size from which the form is chosen by itself
    hop = chain(12, -1.0, True)
    j = 0.5 * np.abs(hop)
    with LanczosEngine() as tj:
        tj.assemble_tj(12, 4, 4, hop, j, j, np.zeros((12, 12)))
        assert tj.layout()["kernel"] == 5
        bad += _mismatches(tj, [(f, KINDS, dict(), 1, None) for f in ("", "_heis")], text_of=TJ_TEXT)
    assert not bad, "\n".join(bad)


# ---- batch boundaries ----------------------------------------------------------------------------------------------------------------------------------
# 17 strings that stay in every sector below and are not identically zero as operators (sites below 3 for the Hubbard sectors)
HUBBARD_POOL = [
    [("n", 0, UP)], [("n", 1, DOWN)], [("c", 0, UP), ("cdagger", 1, UP)], [("c", 1, DOWN), ("cdagger", 2, DOWN)], [("sz", 0, UP)], [("sz", 1, UP), ("sz", 2, UP)],
    [("n", 0, UP), ("n", 1, DOWN)], [("splus", 0, UP), ("sminus", 1, UP)], [("c", 2, UP), ("cdagger", 0, UP)], [("sz", 2, UP), ("c", 2, UP), ("cdagger", 1, UP)],
    [("n", 2, DOWN)], [("c", 0, DOWN), ("cdagger", 0, DOWN)], [("cdagger", 1, UP), ("c", 1, UP)], [("sminus", 2, UP), ("splus", 0, UP)], [("n", 1, UP)],
    [("c", 0, UP), ("c", 1, DOWN), ("cdagger", 2, DOWN), ("cdagger", 1, UP)], [("sz", 0, UP), ("n", 2, UP)],
]
HUBBARD_SKIPPED = {"leaves": [("c", 0, UP), ("n", 1, UP), ("cdagger", 2, DOWN)]}


def _heis_pool(L):
    s = hmp.strings(L)
    pool = [s[k] for k in range(13) if k not in hmp.DEAD + hmp.LEAVES]
    pool += [[("sz", i, UP), ("sz", (i + 3) % L, UP)] for i in range(4)] + [[("splus", i, UP), ("sminus", L - 1 - i, UP)] for i in range(3)]
    return pool, {"leaves": s[hmp.LEAVES[0]], "dead": s[hmp.DEAD[0]]}


# Hubbard (3;1,1): 9 states, the f64 path ends in half a unit; (5;2,2): 100 states.  Heisenberg (7;2): 21 states; (14;7): 3432, the smallest with a high part
CASES = [("hubbard", 3, 1, 1), ("hubbard", 5, 2, 2), ("spin_half", 7, 2, 0), ("spin_half", 14, 7, 0)]


@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("basis,L,nup,ndown", CASES)
def test_batch_boundaries(basis, L, nup, ndown, dtype):
    """many_point_of on lists of 0, 1, 8, 9, 16 and 17 strings with a string that launches nothing at positions 0, 7 and 8 (one that leaves the sector;
    for the Heisenberg basis also a dead one), so the launched strings fill their batches of 8 across those positions: every value is bit for bit the
    value of the same string computed alone, the skipped ones are exactly 0, the empty list gives an empty result."""
    cplx = dtype == "c128"
    if basis == "hubbard":
        pool, skipped = HUBBARD_POOL, HUBBARD_SKIPPED
        n = mp.size(L, (nup, ndown))
        reference = lambda s, bra, ket: mp.many_point(s, L, (nup, ndown), bra, ket)  # noqa: E731
    else:
        pool, skipped = _heis_pool(L)
        n = href.size(L, nup)
        reference = lambda s, bra, ket: hmp.many_point(s, L, nup, bra, ket)  # noqa: E731
    assert len(pool) == 17
    bra, ket = oracle.fill_random(n, 5, cplx), oracle.fill_random(n, 6, cplx)
    # the reference on the CPU: the lists do not compare zeros with zeros
    assert sum(reference(s, bra, ket) != 0 for s in pool[1:7] + pool[9:]) >= 6
    assert all(reference(s, bra, ket) == 0 for s in skipped.values())
    bits = lambda v: np.ascontiguousarray(v).view(np.uint64)  # noqa: E731
    with LanczosEngine(dtype=dtype) as e:
        of = lambda strings: e.many_point_of(strings, L, nup, ndown, bra, ket, basis=basis)  # noqa: E731
        alone = [of([s])[0] for s in pool]
        assert sum(v != 0 for v in alone[1:7] + alone[9:]) >= 6
        empty = of([])
        assert empty.shape == (0,) and empty.dtype == bra.dtype
        for kind, skip in skipped.items():
            assert of([skip])[0] == 0
            for count in (1, 8, 9, 16, 17):
                strings = [skip if k in (0, 7, 8) else pool[k] for k in range(count)]
                got = of(strings)
                assert got.shape == (count,) and got.dtype == bra.dtype
                for k in range(count):
                    if k in (0, 7, 8):
                        assert bits(got[k:k + 1]).tolist() == [0] * (2 if cplx else 1), (kind, count, k)  # +0.0, nothing launched
                    else:
                        assert np.array_equal(bits(got[k:k + 1]), bits(np.array([alone[k]]))), (kind, count, k)
        # and without a skipped string: full batches of the pool itself
        for count in (8, 9, 16, 17):
            assert np.array_equal(bits(of(pool[:count])), bits(np.array(alone[:count]))), count
