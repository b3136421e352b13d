"""The Python front end of the observables on one engine per basis family (L = 6 ring: Hubbard (3, 3), t-J (2, 2), Heisenberg szPlusConst = 3, spin-1
szPlusConst = 6): every refusal the Python layer raises by itself, with its exception type and full message, the keys of the spectral-function
records in their order, and the one cache of sector engines behind both spectral methods.  Every refusal is a host-side check: nothing is launched."""
import numpy as np
import pytest

import oracle
from helpers import chain
from lanczosplusplus_amd import LanczosEngine, LppError

pytestmark = pytest.mark.gpu

L = 6
FAMILIES = ("hubbard", "tj", "spin_half", "spin")
SECTOR = {"hubbard": (3, 3), "tj": (2, 2), "spin_half": (3, 0), "spin": (6, 0)}
TWICE_S = {"hubbard": None, "tj": None, "spin_half": None, "spin": 2}
STATES = {"hubbard": 400, "tj": 90, "spin_half": 20, "spin": 141}
STAYS = {"hubbard": "n", "tj": "n", "spin_half": "sz", "spin": "sz"}  # an operator that keeps the sector
NEED_MODEL = " needs a single-GPU engine set up by assemble_hubbard / setup_hubbard_onthefly / assemble_tj / assemble_heisenberg"
RECORD_KEYS = ["type", "label", "a", "b", "Eg", "weight", "sigma", "modif_norm2", "steps", "sector", "ms_per_step", "assemblies"]


def _assemble(e, family):
    hop = chain(L, -1.0, True)
    j = 0.5 * np.abs(hop)
    if family == "hubbard":
        e.assemble_hubbard(L, 3, 3, hop, np.full(L, 4.0))
    elif family == "tj":
        e.assemble_tj(L, 2, 2, hop, j, j, np.zeros((L, L)))
    else:
        e.assemble_heisenberg(L, SECTOR[family][0], j, j, twiceS=2 if family == "spin" else 1)


@pytest.fixture(scope="module")
def engines():
    """one solved engine per family, the ground state resident"""
    out = {}
    for family in FAMILIES:
        e = LanczosEngine()
        _assemble(e, family)
        (e.keep_states_tj if family == "tj" else e.keep_states)(1)
        e.lanczos(1, want_vectors=False)
        assert e.rows() == STATES[family]
        out[family] = e
    yield out
    for e in out.values():
        e.close()


def _raises(exc, text, call):
    with pytest.raises(exc) as ei:
        call()
    assert type(ei.value) is exc and str(ei.value) == text


RESIDENT = {"two_point": lambda e, **kw: e.two_point("sz", **kw), "weighted_norm2": lambda e, **kw: e.weighted_norm2("sz", np.ones(L), **kw),
            "spectral_function": lambda e, **kw: e.spectral_function("splus", 0, 0, **kw),
            "spectral_function_weighted": lambda e, **kw: e.spectral_function_weighted("splus", np.ones(L), **kw)}


def test_an_engine_without_a_model_is_refused():
    with LanczosEngine() as e:
        A = oracle.hubbard_csr(L, 3, 3, chain(L, -1.0, True), np.full(L, 4.0))
        e.set_csr(A.rowptr, A.colind, A.values)  # a matrix, but no model behind it
        for who, call in RESIDENT.items():
            _raises(LppError, "LPP_ERR_STATE: " + who + NEED_MODEL, lambda: call(e))
        _raises(LppError, "LPP_ERR_STATE: many_point" + NEED_MODEL, lambda: e.many_point(["n?0?0"]))
        _raises(ValueError, "many_point: basis=\"tj\" is for engines set up by assemble_tj", lambda: e.many_point(["n?0?0"], basis="tj"))


@pytest.mark.parametrize("who", sorted(RESIDENT))
def test_the_basis_argument_of_the_resident_state_calls(engines, who):
    call = RESIDENT[who]
    for family in ("hubbard", "tj"):
        _raises(LppError, "LPP_ERR_INVALID: %s: basis=\"spin\" is for engines set up by assemble_heisenberg" % who, lambda: call(engines[family], basis="spin"))
    for family in FAMILIES:
        _raises(ValueError, "%s: unsupported basis 'tj' (None for the engine's own, or \"spin\")" % who, lambda: call(engines[family], basis="tj"))
    _raises(LppError, "LPP_ERR_INVALID: %s: the observables of a Heisenberg model need twiceS = 1 (the reference throws for higher spins)" % who,
            lambda: call(engines["spin"]))


def test_operator_strings_are_refused_by_the_model(engines):
    tj = ("LPP_ERR_INVALID: %s: not for the t-J (TjMultiOrb) model, operator strings are built for the Hubbard product basis; pass basis=\"tj\" for strings in "
          "the t-J basis (sz is then n of the given spin, the many-point convention only)")
    heis = ("LPP_ERR_INVALID: %s: not for the Heisenberg model, operator strings are built for the Hubbard product basis; pass basis=\"spin_half\" for strings "
            "of n, sz, splus, sminus in the spin basis (sz is then the raw 1 - 2 bit = -2 S^z)")
    src = np.zeros(STATES["tj"])
    _raises(LppError, tj % "many_point", lambda: engines["tj"].many_point(["n?0?0"]))
    _raises(LppError, tj % "many_point", lambda: engines["tj"].many_point(["n?0?0"], basis="spin_half"))
    _raises(LppError, tj % "apply_operator_string", lambda: engines["tj"].apply_operator_string([("n", 0, 0)], L, 2, 2, src))
    _raises(LppError, tj % "many_point_of", lambda: engines["tj"].many_point_of(["n?0?0"], L, 2, 2, src, src))
    for family in ("spin_half", "spin"):
        _raises(LppError, heis % "many_point", lambda: engines[family].many_point(["sz?0?0"]))
    _raises(LppError, heis % "apply_operator_string", lambda: engines["spin_half"].apply_operator_string([("n", 0, 0)], L, 3, 0, np.zeros(20)))
    for family in ("hubbard", "spin_half", "spin"):
        _raises(ValueError, "many_point: basis=\"tj\" is for engines set up by assemble_tj", lambda: engines[family].many_point(["n?0?0"], basis="tj"))
    _raises(LppError, "LPP_ERR_INVALID: many_point: basis=\"spin_half\" is for engines set up by assemble_heisenberg (twiceS = 1)",
            lambda: engines["hubbard"].many_point(["sz?0?0"], basis="spin_half"))
    _raises(LppError, "LPP_ERR_INVALID: many_point: the observables of a Heisenberg model need twiceS = 1 (the reference throws for higher spins)",
            lambda: engines["spin"].many_point(["sz?0?0"], basis="spin_half"))
    _raises(ValueError, "unsupported basis 'spin' for operator strings (one of hubbard, spin_half, tj)", lambda: engines["spin"].many_point(["sz?0?0"], basis="spin"))
    _raises(ValueError, "basis=\"spin_half\" has convention=\"many_point\" only, not 'measure'",
            lambda: engines["spin_half"].many_point([[("sz", 0, 0, False)]], convention="measure", basis="spin_half"))


def test_spectral_functions_refuse_before_any_sector_engine(engines):
    hub, tj = engines["hubbard"], engines["tj"]
    before = hub.sector_assemblies, tj.sector_assemblies
    _raises(LppError, "LPP_ERR_INVALID: spectral_function: operators that stay in the sector (n, sz) are not supported", lambda: hub.spectral_function("n", 0, 0))
    _raises(LppError, "LPP_ERR_INVALID: spectral_function: splus / sminus of the t-J basis take spin UP (the reference ranks words outside the basis otherwise)",
            lambda: tj.spectral_function("splus", 0, 0, spin=1))
    _raises(LppError, "LPP_ERR_INVALID: spectral_function_weighted: splus / sminus of the t-J basis take spin UP",
            lambda: tj.spectral_function_weighted("sminus", np.ones(L), spin=1))
    assert (hub.sector_assemblies, tj.sector_assemblies) == before
    with LanczosEngine() as e:  # a model, but no solve yet
        _assemble(e, "hubbard")
        _raises(LppError, "LPP_ERR_STATE: spectral_function: run lanczos() first (after keep_states) or pass energy", lambda: e.spectral_function("c", 0, 0))
        _raises(LppError, "LPP_ERR_STATE: spectral_function_weighted: run lanczos() first (after keep_states) or pass energy",
                lambda: e.spectral_function_weighted("c", np.ones(L)))
        assert e.sector_assemblies == 0


@pytest.mark.parametrize("family", FAMILIES)
def test_vector_lengths_are_checked(family):
    """src and out of apply_operator, apply_operator_sum and (the three string families) apply_operator_string, for an operator that keeps the sector"""
    nup, ndown = SECTOR[family]
    n, op, t = STATES[family], STAYS[family], TWICE_S[family]
    kw = dict(basis=family) if t is None else dict(basis=family, twiceS=t)
    src_text = "src does not have the length of sector (%d, %d)" % (nup, ndown)
    with LanczosEngine() as e:  # (these calls need no matrix)
        _raises(ValueError, src_text, lambda: e.apply_operator(op, 0, 0, L, nup, ndown, np.zeros(n + 1), **kw))
        _raises(ValueError, "out does not have the length of sector (%d, %d)" % (nup, ndown),
                lambda: e.apply_operator(op, 0, 0, L, nup, ndown, np.zeros(n), out=np.zeros(n - 1), **kw))
        _raises(ValueError, src_text, lambda: e.apply_operator_sum(op, 0, np.ones(L), L, nup, ndown, np.zeros(n - 1), **kw))
        _raises(ValueError, "out does not have the length of the operator's sector",
                lambda: e.apply_operator_sum(op, 0, np.ones(L), L, nup, ndown, np.zeros(n), out=np.zeros(n + 1), **kw))
        if family != "spin":
            _raises(ValueError, src_text, lambda: e.apply_operator_string([(op, 0, 0)], L, nup, ndown, np.zeros(n + 1), basis=family))
            _raises(ValueError, "out does not have the length of sector (%s)" % ("%d" % nup if family == "spin_half" else "%d, %d" % (nup, ndown)),
                    lambda: e.apply_operator_string([(op, 0, 0)], L, nup, ndown, np.zeros(n), out=np.zeros(n + 1), basis=family))
        else:
            _raises(ValueError, "unsupported basis 'spin' for operator strings (one of hubbard, spin_half, tj)",
                    lambda: e.apply_operator_string([(op, 0, 0)], L, nup, ndown, np.zeros(n), basis=family))


@pytest.mark.parametrize("family", FAMILIES)
def test_records_and_the_shared_sector_engines(engines, family):
    """both spectral methods give records with today's keys in today's order, and assemble one sector engine per distinct sector between them"""
    e = engines[family]
    op = "splus" if family in ("spin_half", "spin") else "c"
    kw = dict(max_steps=20, basis="spin" if family == "spin" else None)
    plain = e.spectral_function(op, 0, 0, **kw)
    assert [r["type"] for r in plain] == [0, 1] and all(list(r) == RECORD_KEYS for r in plain)
    sectors = {r["sector"] for r in plain}
    assert len(sectors) == 2 and e.sector_assemblies == 2 and [r["assemblies"] for r in plain] == [1, 2]
    weighted = e.spectral_function_weighted(op, np.ones(L), **kw)
    assert [r["type"] for r in weighted] == [0, 1] and all(list(r) == RECORD_KEYS[:1] + ["part"] + RECORD_KEYS[1:] and r["part"] is None for r in weighted)
    assert {r["sector"] for r in weighted} == sectors and e.sector_assemblies == 2  # the same two engines
    stay = e.spectral_function_weighted(STAYS[family], np.arange(1.0, L + 1), **kw)  # the state's own sector, on an engine of its own
    assert {r["sector"] for r in stay} == {SECTOR[family]} and e.sector_assemblies == 3 == len(e._sectors)
    assert sorted(e._sectors) == sorted(sectors | {SECTOR[family]})
