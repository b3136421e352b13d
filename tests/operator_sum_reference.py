"""The site-weighted operator sum |phi> = sum_r f_r A_r |src> as a plain loop over the sites of the per-site restatements of the reference
(obs_reference / tj_obs_reference / heis_obs_reference .acc_modified_state*), and the dense resolvent the continued fractions approximate.
A_r is Engine::accModifiedState's operator in the two fermion bases (sz = n_up/2 - n_down/2) and the raw operator of the Heisenberg basis
(sz = 1 - 2 bit), as the engine's docstrings state.  Nothing here comes from the engine under test."""
from math import comb

import numpy as np

import obs_reference as ref
from obs_reference import DOWN, UP  # noqa: F401

FUSED_OPS = ("c", "cdagger", "n", "sz")
# the sectors the issue names: odd lengths; c up leaves one up word (W = L); one block each way
HOST_SECTORS = ((5, 2, 3), (6, 1, 3), (6, 3, 0), (6, 3, 6))


def width(op, spin, L, new_parts):
    """sources per destination of the fused plan: L - n or n of the moved species' destination count for c / cdagger, 1 for n / sz"""
    if op in ("n", "sz"):
        return 1
    n = new_parts[1] if spin == DOWN else new_parts[0]
    return L - n if op == "c" else n


def hubbard_sum(op, spin, L, parts, weights, src, out=None):
    """(z, new parts) or (None, None); complex weights give a complex z"""
    new = ref.new_sector(op, spin, L, *parts)
    if new is None:
        return None, None
    w = np.asarray(weights)
    dtype = np.result_type(w.dtype, np.asarray(src).dtype, np.float64)
    z = np.zeros(comb(L, new[0]) * comb(L, new[1]), dtype) if out is None else np.array(out, dtype)
    for r in range(L):
        if w[r] != 0:
            ref.acc_modified_state(z, op, L, parts, new, src, r, spin, w[r])
    return z, new


def tj_sum(op, spin, L, parts, weights, src):
    import tj_obs_reference as tj
    new = tj.new_sector(op, spin, L, *parts)
    if new is None:
        return None, None
    w = np.asarray(weights)
    z = np.zeros(tj.size(L, *new), np.result_type(w.dtype, np.asarray(src).dtype, np.float64))
    for r in range(L):
        if w[r] != 0:
            tj.acc_modified_state(z, op, L, parts, new, src, r, spin, w[r])
    return z, new


def heis_sum(op, spin, L, m, weights, src):
    import heis_obs_reference as heis
    new = heis.new_sector(op, spin, L, m)
    w = np.asarray(weights)
    z = np.zeros(heis.size(L, new), np.result_type(w.dtype, np.asarray(src).dtype, np.float64))
    for r in range(L):
        if w[r] != 0:
            heis.acc_modified_state_(z, op, L, m, new, src, r, spin, w[r])
    return z, new


def bound(W, weights, src):
    """per element: first-order rounding of a W-term sum of products on both sides, 4 (W + 2) eps sum|f| max|src| (derived, not measured)"""
    return 4 * (W + 2) * 2.2e-16 * float(np.sum(np.abs(weights))) * float(np.max(np.abs(src)))


def momentum_weights(L, m):
    """chain momentum q = 2 pi m / L"""
    return np.exp(2j * np.pi * m * np.arange(L) / L) / np.sqrt(L)


def dense_resolvent(Hd, eg, phi, z, sigma=-1.0):
    """<phi| (z + sigma (H - Eg))^-1 |phi> by a dense solve per frequency (continued_fraction's convention)"""
    n = len(phi)
    A = sigma * (Hd - eg * np.eye(n))
    return np.array([np.vdot(phi, np.linalg.solve(zz * np.eye(n) + A, phi)) for zz in np.atleast_1d(z)])
