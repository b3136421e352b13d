"""The host-only front end of the observables, for all four basis families at once (no GPU): sector sizes against a brute-force count of the words and
against the n_dst of the family's own plan call, new_parts against the literal rules of the four *_obs_reference.py restatements, and the refusals the
Python layer raises by itself, on their full text."""
import itertools

import pytest

import heis_obs_reference
import heis_spin_obs_reference
import obs_reference
import tj_obs_reference
from lanczosplusplus_amd import LppError, new_parts
from lanczosplusplus_amd.engine import (OP_NAMES, operator_plan, operator_plan_heis, operator_plan_heis_spin, operator_plan_tj, operator_string_plan,
                                        sector_size)

SIZES = (1, 2, 5)


def _sectors(basis, L):
    """every admissible (nup, ndown, twiceS) of the basis on L sites"""
    if basis == "hubbard":
        return [(u, d, None) for u in range(L + 1) for d in range(L + 1)]
    if basis == "tj":
        return [(u, d, None) for u in range(L + 1) for d in range(L + 1 - u)]
    if basis == "spin_half":
        return [(m, 0, None) for m in range(L + 1)]
    return [(m, 0, t) for t in (2, 3) for m in range(L * t + 1)]


def _count_words(basis, L, nup, ndown, twiceS):
    """the words of the sector, one by one"""
    if basis == "spin":
        return sum(1 for w in itertools.product(range(twiceS + 1), repeat=L) if sum(w) == nup)
    ups = [u for u in range(1 << L) if bin(u).count("1") == nup]
    if basis == "spin_half":
        return len(ups)
    downs = [d for d in range(1 << L) if bin(d).count("1") == ndown]
    return sum(1 for u in ups for d in downs if basis == "hubbard" or not (u & d))


def _plan_n_dst(basis, L, nup, ndown, twiceS):
    """n_dst of the family's plan call for an operator that stays in the sector (n, in the spin bases sz), None where the plan has no sector"""
    if basis == "hubbard":
        p = operator_plan("n", 0, 0, L, nup, ndown)
        return None if p is None else len(p["table_up"]) * len(p["table_down"])
    if basis == "tj":
        p = operator_plan_tj("n", 0, 0, L, nup, ndown)
        return None if p is None else len(p["action"])
    if basis == "spin_half":
        return len(operator_plan_heis("sz", 0, 0, L, nup)["action"])
    return len(operator_plan_heis_spin("sz", 0, L, twiceS, nup)["action"])


@pytest.mark.parametrize("basis", ["hubbard", "tj", "spin_half", "spin"])
def test_sector_size_counts_the_words(basis):
    seen = 0
    for L in SIZES:
        for nup, ndown, t in _sectors(basis, L):
            want = _count_words(basis, L, nup, ndown, t)
            assert sector_size(L, nup, ndown, basis=basis, twiceS=t) == want, (L, nup, ndown, t)
            n_dst = _plan_n_dst(basis, L, nup, ndown, t)
            if n_dst is not None:
                assert n_dst == want, (L, nup, ndown, t)
                seen += 1
    assert seen >= len(SIZES)


def _rule(basis, op, spin, L, nup, ndown, twiceS):
    """the new sector as new_parts reports it, None for `false`; raises where the reference throws"""
    if basis == "hubbard":
        return obs_reference.has_new_parts(op, spin, L, nup, ndown)
    if basis == "tj":
        return tj_obs_reference.has_new_parts(op, spin, L, nup, ndown)
    if basis == "spin_half":
        new = heis_obs_reference.has_new_parts(op, spin, L, nup)
    else:
        new = heis_spin_obs_reference.has_new_parts(op, L, twiceS, nup, spin)
    return None if new is None else (new, 0)


@pytest.mark.parametrize("basis", ["hubbard", "tj", "spin_half", "spin"])
def test_new_parts_follows_the_literal_rule(basis):
    refused = answered = 0
    for L in SIZES:
        for nup, ndown, t in _sectors(basis, L):
            for op in OP_NAMES:
                for spin in (0, 1):
                    try:
                        want = _rule(basis, op, spin, L, nup, ndown, t)
                    except Exception:
                        with pytest.raises(LppError) as ei:
                            new_parts(op, spin, L, nup, ndown, basis=basis, twiceS=t)
                        assert ei.value.status == 1, (L, nup, ndown, t, op, spin)
                        refused += 1
                        continue
                    got = new_parts(op, spin, L, nup, ndown, basis=basis, twiceS=t)
                    assert got == (None if want is None else tuple(want)), (L, nup, ndown, t, op, spin)
                    answered += 1
    assert refused and answered


def test_refusals_of_the_python_layer():
    for call in (lambda: sector_size(3, 1, 1, basis="kagome"), lambda: new_parts("c", 0, 3, 1, 1, basis="kagome")):
        with pytest.raises(ValueError) as ei:
            call()
        assert str(ei.value) == "unsupported basis 'kagome' (one of hubbard, tj, spin_half, spin)"
    for call in (lambda: sector_size(3, 1, 0, basis="spin"), lambda: new_parts("splus", 0, 3, 1, 0, basis="spin")):
        with pytest.raises(ValueError) as ei:
            call()
        assert str(ei.value) == "basis=\"spin\" needs twiceS"
    with pytest.raises(ValueError) as ei:
        operator_string_plan([("n", 0, 0)], 2, 1, 1, convention="bracket")
    assert str(ei.value) == "unsupported convention 'bracket' (one of many_point, measure)"
    with pytest.raises(ValueError) as ei:
        operator_string_plan("n?0?0", 2, 1, 1, convention="measure")
    assert str(ei.value) == "text strings are the -M form; pass measure operators as (label, site, dof, transpose)"
