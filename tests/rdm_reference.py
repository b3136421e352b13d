"""numpy restatement of the reference's reduced density matrix (src/Engine/ReducedDensityMatrix.h) for the tests of the GPU path.

`literal` is build() / unpackHubbard / unpackHeisenberg line by line, with the O(N^2) double loop: use it for N <= ~1000 only.
`plan` and `blocks` are the block form the engine computes, derived here from the basis words alone (oracle.hubbard_basis_words,
oracle.heis_basis): nothing is shared with the planner under test.
"""
import numpy as np

import oracle


def species_words(L, nup, ndown, basis="hubbard"):
    """(up words, down words) of the species, ascending; one species for spin_half (the down species is the empty word)"""
    if basis == "spin_half":
        return oracle.heis_basis(L, 1, nup).astype(np.int64), np.zeros(1, np.int64)
    up, dn = oracle.hubbard_basis_words(L, nup, ndown)
    n_up = len(oracle.onespin_basis(L, nup))
    return up[:n_up].astype(np.int64), dn[::n_up].astype(np.int64)


def state_words(L, nup, ndown, basis="hubbard"):
    """(up word, down word) of every state in the basis order"""
    uw, dw = species_words(L, nup, ndown, basis)
    return np.tile(uw, len(dw)), np.repeat(dw, len(uw))


def literal(L, nup, ndown, split, psi, basis="hubbard"):
    """ReducedDensityMatrix::build (:65-76) with unpackHubbard (:104-123) / unpackHeisenberg (:90-102)"""
    up, dn = state_words(L, nup, ndown, basis)
    hilbert = len(up)
    assert len(psi) == hilbert
    one_site = 2 if basis == "spin_half" else 4
    row = one_site ** split
    nabits, nbbits = split, L - split
    rdm = np.zeros((row, row), psi.dtype)

    def unpack(ind):
        words = [int(up[ind])] if basis == "spin_half" else [int(up[ind]), int(dn[ind])]
        a, b = [], []
        for w in words:
            mask = (1 << nabits) - 1
            a.append(w & mask)
            mask = ((1 << nbbits) - 1) << nabits
            b.append((w & mask) >> nabits)
        if basis == "spin_half":
            return a[0], b[0]
        return a[0] + a[1] * (1 << nabits), b[0] + b[1] * (1 << nbbits)

    pairs = [unpack(i) for i in range(hilbert)]
    for i in range(hilbert):
        for j in range(hilbert):
            if pairs[i][1] != pairs[j][1]:
                continue
            rdm[pairs[i][0], pairs[j][0]] += np.conj(psi[i]) * psi[j]
    return rdm


def _classes(words, split):
    """{k: (low words ascending, run-start ranks of the high words ascending)} of one species"""
    lo, hi = words & ((1 << split) - 1), words >> split
    pop = np.array([bin(int(x)).count("1") for x in lo])
    out = {}
    for k in sorted(set(pop.tolist())):
        idx = np.nonzero(pop == k)[0]
        his = np.unique(hi[idx])
        starts = np.array([idx[hi[idx] == t][0] for t in his], np.int64)
        out[k] = (np.unique(lo[idx]), starts)
    return out


def plan(L, nup, ndown, split, basis="hubbard"):
    """blocks in ascending (k_down, k_up): dicts of k_up, k_down, dim_up, dim_down, dim, env_up, env_down, terms, offset, alpha, starts_up, starts_down"""
    uw, dw = species_words(L, nup, ndown, basis)
    cu, cd = _classes(uw, split), _classes(dw, split)
    blocks, off = [], 0
    for kd in sorted(cd):
        for ku in sorted(cu):
            lo_u, s_u = cu[ku]
            lo_d, s_d = cd[kd]
            d = len(lo_u) * len(lo_d)
            alpha = (lo_u[None, :] + (lo_d[:, None] << split)).reshape(-1)
            blocks.append(dict(k_up=ku, k_down=kd, dim_up=len(lo_u), dim_down=len(lo_d), dim=d, env_up=len(s_u), env_down=len(s_d),
                               terms=len(s_u) * len(s_d), offset=off, alpha=alpha, starts_up=s_u, starts_down=s_d))
            off += d * d
    return dict(blocks=blocks, total=off, states=len(uw) * len(dw), n_up=len(uw))


def blocks(L, nup, ndown, split, psi, basis="hubbard"):
    """[(k_up, k_down, alpha, rho)] with rho = conj(V) V^T, V[r, b] = psi[(s_up[t_up] + a_up) + (s_down[t_down] + a_down) * N_up]"""
    p = plan(L, nup, ndown, split, basis)
    assert len(psi) == p["states"]
    out = []
    for b in p["blocks"]:
        iu = np.arange(b["dim_up"])[:, None] + b["starts_up"][None, :]  # [a_up, t_up]
        idn = (np.arange(b["dim_down"])[:, None] + b["starts_down"][None, :]) * p["n_up"]  # [a_down, t_down]
        idx = iu[None, :, None, :] + idn[:, None, :, None]  # [a_down, a_up, t_down, t_up]
        v = psi[idx.reshape(b["dim"], b["terms"])]
        out.append((b["k_up"], b["k_down"], b["alpha"], v.conj() @ v.T))
    return out


def scatter(blks, rows, dtype):
    """the reference's dense matrix from the blocks"""
    out = np.zeros((rows, rows), dtype)
    for _, _, alpha, m in blks:
        out[np.ix_(alpha, alpha)] = m
    return out


def tolerance(rho, terms):
    """K * 2^-52 * max_r rho[r, r]: K products and K - 1 additions, every term bounded by sqrt(rho_rr rho_cc) -- any summation order meets it"""
    return terms * 2.0 ** -52 * float(np.max(np.real(np.diag(rho))))
