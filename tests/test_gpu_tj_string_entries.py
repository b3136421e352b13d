"""The five operator-string entry points of the t-J family in the C ABI (lpp_engine_apply_string_tj, _tj_host, lpp_engine_many_point_tj, _tj_host,
lpp_engine_bench_string_dot_tj), called below the Python layer: (status, text) of every refusal they make before they launch, in the order of the
shared front's checks -- null argument, the engine and the convention, the list, the count of a bench, the sector, the resident states -- and that a
hole-major engine is served.  The table has the shape of tests/test_gpu_string_entries.py, which pins the other ten."""
import ctypes as C

import numpy as np
import pytest

from helpers import chain
from lanczosplusplus_amd import LanczosEngine

pytestmark = pytest.mark.gpu

UP, DOWN = 0, 1
OP = dict(c=1, sz=2, cdagger=3, n=4, splus=5, sminus=6)
KINDS = ("apply", "apply_host", "many_point", "many_point_host", "bench")
NAME = dict(apply="lpp_engine_apply_string_tj", apply_host="lpp_engine_apply_string_tj_host", many_point="lpp_engine_many_point_tj",
            many_point_host="lpp_engine_many_point_tj_host", bench="lpp_engine_bench_string_dot_tj")
LISTS = ("many_point", "many_point_host", "bench")
APPLY = ("apply", "apply_host")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(e, valid, kind, **changes):
    """(status, lpp_last_error()) of one entry point with the arguments of `valid` but for `changes`.  null=True: the result / has / ms pointer is NULL.
    The device-vector apply gets no vectors: every refusal below comes before they are read."""
    a = dict(valid, bra_state=0, ket_state=0, warmup=0, iters=1, null=False)
    a.update(changes)
    ops, sites, spins = (np.array(a[k], np.int32) for k in ("ops", "sites", "spins"))
    flags, off = np.zeros_like(ops), np.array(a["off"], np.int64)
    fn = getattr(e._lib, NAME[kind])
    sector = (a["L"], a["nup"], a["ndown"])
    x, y = np.ones(a["n"]), np.ones(a["n"])
    if kind in APPLY:
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


PLANNER = "t-J operator string"
BAD_SECTOR_TEXT = ": bad sites / sector (nup + ndown <= sites <= 30)"
NINE = dict(ops=[OP["n"]] * 9, sites=[0] * 9, spins=[UP] * 9, off=list(range(10)))
LEAVES_TEXT = "@: a string that is identically zero, leads to no sector or leaves the sector launches nothing"
MEASURE_TEXT = "@: the t-J basis has the many-point convention only (RahulOperator on this basis is not restated)"
SEVENTEEN = dict(ops=[OP["n"]] * 17, sites=[0] * 17, spins=[UP] * 17)

ROWS = [
    (APPLY + ("many_point", "many_point_host"), dict(null=True), 1, "@: null argument"),
    (("bench",), dict(null=True), 1, "@: bad argument"),
    (("bench",), dict(iters=0), 1, "@: bad argument"),
    (KINDS, dict(conv=1), 1, MEASURE_TEXT),  # the measure convention on each
    (APPLY, dict(nops=0), 1, PLANNER + ": 1 to 16 operators per string"),
    (APPLY, dict(nops=17, **SEVENTEEN), 1, PLANNER + ": 1 to 16 operators per string"),
    (LISTS, dict(off=[0, 0]), 1, "@: 1 to 16 operators per string"),
    (LISTS, dict(off=[0, 17], **SEVENTEEN), 1, "@: 1 to 16 operators per string"),
    (LISTS, dict(off=[-1, 0]), 1, "@: 1 to 16 operators per string"),
    (("bench",), dict(off=[0], nstrings=0), 1, "@: 1 to 8 strings (one launch)"),
    (("bench",), NINE, 1, "@: 1 to 8 strings (one launch)"),
    (("bench",), dict(NINE, nup=9), 1, "@: 1 to 8 strings (one launch)"),  # the count before the sector
    (APPLY, dict(nup=9), 1, PLANNER + BAD_SECTOR_TEXT),
    (LISTS, dict(nup=9), 1, "@" + BAD_SECTOR_TEXT),
    (LISTS, dict(L=31), 1, "@" + BAD_SECTOR_TEXT),
    (("many_point",), dict(bra_state=3), 5, "@: no such resident state (lpp_engine_keep_states before lpp_engine_lanczos)"),
    (("many_point",), dict(ket_state=3), 5, "@: no such resident state (lpp_engine_keep_states before lpp_engine_lanczos)"),
    (("many_point",), dict(nup=1, ndown=1), 1, "@: (sites, nup, ndown) is not the sector of the resident states"),
    # the planner's refusals reach every entry point with its own words
    (KINDS, dict(ops=[0]), 1, PLANNER + ": unknown operator (LPP_OP_*)"),
    (KINDS, dict(spins=[2]), 1, PLANNER + ": spin must be LPP_SPIN_UP or LPP_SPIN_DOWN"),
    (KINDS, dict(sites=[99]), 1, PLANNER + ": site out of range"),
    (KINDS, dict(ops=[OP["splus"]], spins=[DOWN]), 1, None),
    # the bench: strings that stay -- one that leaves, one that is dead, one without a sector
    (("bench",), dict(ops=[OP["c"]]), 1, LEAVES_TEXT),
    (("bench",), dict(ops=[OP["n"], OP["n"]], sites=[0, 0], spins=[UP, DOWN], off=[0, 2]), 1, LEAVES_TEXT),
    # what is served, so that a refusal above is the row's doing and not the harness's
    (("apply_host", "many_point", "many_point_host", "bench"), dict(), 0, None),
]


def _mismatches(e, valid, rows):
    bad = []
    for kinds, changes, status, text in rows:
        for kind in kinds:
            st, msg = _call(e, valid, kind, **changes)
            want = None if text is None else text.replace("@", NAME[kind])
            if st != status or (want is not None and msg != want):
                bad.append("%s %r: got (%d, %r), pinned (%d, %r)" % (NAME[kind], changes, st, msg, status, want))
    return bad


@pytest.mark.parametrize("layout", ["0", "1"])
def test_tj_string_entry_refusals_are_pinned(layout, monkeypatch):
    """on the general layout of an 8-site ring (3,3), 560 states, and on a hole-major engine (12;4,4), which the _tj entry points serve"""
    L, nup, ndown, n = (12, 4, 4, 34650) if layout == "1" else (8, 3, 3, 560)
    monkeypatch.setenv("LPP_TJ_LAYOUT", layout)
    hop = chain(L, -1.0, True)
    j = 0.5 * np.abs(hop)
    valid = dict(conv=0, ops=[OP["n"]], sites=[0], spins=[UP], off=[0, 1], L=L, nup=nup, ndown=ndown, n=n)
    with LanczosEngine() as e:
        e.assemble_tj(L, nup, ndown, hop, j, j, np.zeros((L, L)))
        assert (e.layout()["kernel"] == 5) == (layout == "1") and e.rows() == n
        e.keep_states_tj(1)
        e.lanczos(1, want_vectors=False)
        bad = _mismatches(e, valid, ROWS)
    assert not bad, "\n".join(bad)
