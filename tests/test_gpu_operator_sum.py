"""-m gpu: site-weighted operator sums |phi> = sum_r f_r A_r |src> (one fused launch in the Hubbard basis and for the Heisenberg sz, the chain of
one-site launches elsewhere), the static structure factor <phi|phi> and the continued fractions of the momentum-resolved spectral functions, against
the per-site CPU restatements of the reference summed over the sites (tests/operator_sum_reference.py) and the oracle's decomposition."""
import ctypes as C
import os
import re
import subprocess
import threading

import numpy as np
import pytest
import torch  # before any engine opens the GPU: the threads of the multi-rank test drive torch's streams on the same runtime

import heis_obs_reference as href
import obs_reference as ref
import operator_sum_reference as sref
import oracle
from helpers import chain, rel
from lanczosplusplus_amd import LanczosEngine, LppError, _capi, continued_fraction, geometry, operator_sum_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "lanczosplusplus_amd", "host", "lanczos")
GOLD = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

# L = 8 ring sectors, then the odd, the W = L and the one-block sectors of the host tests
SECTORS = ((8, 4, 4), (8, 4, 3)) + sref.HOST_SECTORS


def _ring(L):
    return chain(L, -1.0, True)


def _weight_sets(L, cplx, seed):
    rng = np.random.default_rng(seed)
    rnd = rng.standard_normal(L) + (1j * rng.standard_normal(L) if cplx else 0)
    mom = sref.momentum_weights(L, 1)  # q = 2 pi / L; an f64 engine takes its cosine part
    holes = rnd.copy()
    holes[::2] = 0
    single = np.zeros(L, rnd.dtype)
    single[L - 2] = rnd[L - 2]
    return {"random": rnd, "momentum": mom if cplx else mom.real.copy(), "zeros": holes, "single": single}


@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("L,nup,ndown", SECTORS)
def test_fused_equals_reference(dtype, L, nup, ndown):
    """c, cdagger, n, sz of both spins under four kinds of weights: every element within 4 (W + 2) eps sum|f| max|src| of the site loop on the CPU;
    destinations none of whose sources carries a weight are exactly 0; out= accumulates; two calls give the same bits; a single weight reproduces
    apply_operator (sz: half the raw operator, which is 2 S^z there)."""
    cplx = dtype == "c128"
    parts = (nup, ndown)
    n = ref.comb(L, nup) * ref.comb(L, ndown)
    src = oracle.fill_random(n, 11, cplx)
    seen_dead = 0
    with LanczosEngine(dtype=dtype) as e:
        for op in sref.FUSED_OPS:
            for spin in (ref.UP, ref.DOWN):
                new = ref.new_sector(op, spin, L, *parts)
                for name, f in _weight_sets(L, cplx, 3 * L + nup).items():
                    z, got = e.apply_operator_sum(op, spin, f, L, nup, ndown, src)
                    if new is None:
                        assert z is None and got is None
                        continue
                    want, _ = sref.hubbard_sum(op, spin, L, parts, f, src)
                    W = sref.width(op, spin, L, new)
                    tol = sref.bound(W, f, src)
                    assert got == new and len(z) == len(want)
                    assert np.max(np.abs(z - want)) <= tol, (op, spin, name, np.max(np.abs(z - want)), tol)
                    plan = operator_sum_plan(op, spin, L, nup, ndown, f)
                    dead = np.all(plan["factor"] == 0, axis=1)
                    assert np.all(z[dead] == 0), (op, spin, name)
                    seen_dead += int(dead.sum())
                    z2, _ = e.apply_operator_sum(op, spin, f, L, nup, ndown, src, out=z.copy())
                    assert np.max(np.abs(z2 - 2 * want)) <= 2 * tol, (op, spin, name)
                    z3, _ = e.apply_operator_sum(op, spin, f, L, nup, ndown, src)
                    assert np.array_equal(z3.view(np.uint64), z.view(np.uint64)), (op, spin, name)
                    if name == "single":
                        r = L - 2
                        one, _ = e.apply_operator(op, r, spin, L, nup, ndown, src, factor=f[r] * (0.5 if op == "sz" else 1.0))
                        assert np.max(np.abs(z - one)) <= tol, (op, spin)
    assert seen_dead > 0  # the exact zeros were checked on something


@pytest.mark.parametrize("dtype", ["f64", "c128"])
def test_multi_tile(dtype):
    """L = 12, (6, 5): 731808 elements -- several hundred tiles, one per block, and block boundaries inside a tile; c up and c down, the same bound
    (the grid stride needs more tiles than 32 blocks per CU: test_grid_stride)"""
    L, nup, ndown = 12, 6, 5
    cplx = dtype == "c128"
    n = ref.comb(L, nup) * ref.comb(L, ndown)
    src = oracle.fill_random(n, 5, cplx)
    f = _weight_sets(L, cplx, 99)["random"]
    with LanczosEngine(dtype=dtype) as e:
        for spin in (ref.UP, ref.DOWN):
            z, new = e.apply_operator_sum("c", spin, f, L, nup, ndown, src)
            want, wnew = sref.hubbard_sum("c", spin, L, (nup, ndown), f, src)
            assert new == wnew
            tol = sref.bound(sref.width("c", spin, L, new), f, src)
            assert np.max(np.abs(z - want)) <= tol, (spin, np.max(np.abs(z - want)), tol)


def test_grid_stride(monkeypatch):
    """c128, L = 14, (7, 7): 1.03e7 destination units, more than the 8192 blocks of 1024 units a grid holds at most (32 blocks per CU, 256 CUs), so
    blocks take a second tile through the grid stride.  The reference is the chain of one-site launches on the GPU (a CPU site loop over 1.2e7
    states takes a minute), the same bound per element."""
    L, nup, ndown = 14, 7, 7
    src = oracle.fill_random(ref.comb(L, nup) * ref.comb(L, ndown), 19, True)
    f = _weight_sets(L, True, 77)["random"]
    fused = {}
    with LanczosEngine(dtype="c128") as e:
        for spin in (ref.UP, ref.DOWN):
            fused[spin] = e.apply_operator_sum("c", spin, f, L, nup, ndown, src)[0]
            assert len(fused[spin]) > 32 * 256 * 1024
    monkeypatch.setenv("LPP_OBS_SUM_CHAIN", "1")
    with LanczosEngine(dtype="c128") as e:
        for spin, z in fused.items():
            zc, new = e.apply_operator_sum("c", spin, f, L, nup, ndown, src)
            tol = sref.bound(sref.width("c", spin, L, new), f, src)
            assert np.max(np.abs(z - zc)) <= tol, (spin, np.max(np.abs(z - zc)), tol)


@pytest.mark.parametrize("dtype", ["f64", "c128"])
def test_fused_equals_chain(dtype, monkeypatch):
    """LPP_OBS_SUM_CHAIN=1 on a second engine forces the chain of one-site launches: the same numbers to the same bound"""
    L, nup, ndown = 8, 4, 3
    cplx = dtype == "c128"
    src = oracle.fill_random(ref.comb(L, nup) * ref.comb(L, ndown), 17, cplx)
    f = _weight_sets(L, cplx, 41)["random"]
    fused = {}
    with LanczosEngine(dtype=dtype) as e:
        for op in sref.FUSED_OPS:
            for spin in (ref.UP, ref.DOWN):
                fused[op, spin] = e.apply_operator_sum(op, spin, f, L, nup, ndown, src)[0]
    monkeypatch.setenv("LPP_OBS_SUM_CHAIN", "1")
    with LanczosEngine(dtype=dtype) as e:
        for (op, spin), z in fused.items():
            zc, new = e.apply_operator_sum(op, spin, f, L, nup, ndown, src)
            tol = sref.bound(sref.width(op, spin, L, new), f, src)
            assert np.max(np.abs(z - zc)) <= tol, (op, spin, np.max(np.abs(z - zc)), tol)
        ms, by = e.bench_operator_sum("c", ref.UP, f, L, nup, ndown, warmup=1, iters=2)
        assert ms > 0 and by == (16 if cplx else 8) * (ref.comb(L, 3) * ref.comb(L, 3) + ref.comb(L, 4) * ref.comb(L, 3))


@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("L,m", [(12, 6), (12, 5), (14, 7), (15, 6)])
def test_heisenberg(dtype, L, m, monkeypatch):
    """the fused raw sz against the site loop over heis_obs_reference, the same through the chain, and splus through the chain.  L = 12 is one run of
    equal high part (the word's cut is at 12 bits); L = 14 has 4 runs and L = 15 (an odd length, 5005 states) 8: the weights of the high sites
    (k_obs_sum_hi_heis, hi[run]), the run search and a unit of two f64 elements that straddles two runs"""
    cplx = dtype == "c128"
    src = oracle.fill_random(href.size(L, m), 23, cplx)
    f = _weight_sets(L, cplx, 7 + m)["random"]
    tol = sref.bound(L, f, src)  # the factor of an element is a sum over all L sites
    with LanczosEngine(dtype=dtype) as e:
        z, new = e.apply_operator_sum("sz", 0, f, L, m, 0, src, basis="spin_half")
        want, _ = sref.heis_sum("sz", 0, L, m, f, src)
        assert new == (m, 0) and np.max(np.abs(z - want)) <= tol, (np.max(np.abs(z - want)), tol)
        z2, _ = e.apply_operator_sum("sz", 0, f, L, m, 0, src, basis="spin_half")
        assert np.array_equal(z.view(np.uint64), z2.view(np.uint64))
        zp, newp = e.apply_operator_sum("splus", 0, f, L, m, 0, src, basis="spin_half")
        wantp, wnew = sref.heis_sum("splus", 0, L, m, f, src)
        assert newp == (wnew, 0) and np.max(np.abs(zp - wantp)) <= tol
        with pytest.raises(LppError):
            e.apply_operator_sum("c", 0, f, L, m, 0, src, basis="spin_half")  # refused where apply_operator refuses
    monkeypatch.setenv("LPP_OBS_SUM_CHAIN", "1")
    with LanczosEngine(dtype=dtype) as e:
        zc, _ = e.apply_operator_sum("sz", 0, f, L, m, 0, src, basis="spin_half")
        assert np.max(np.abs(zc - z)) <= tol


def test_tj_chain():
    """t-J, 8 sites (3, 3): c of both spins through the chain against the site loop over tj_obs_reference"""
    import tj_obs_reference as tj
    L, parts = 8, (3, 3)
    src = oracle.fill_random(tj.size(L, *parts), 29, True)
    f = _weight_sets(L, True, 13)["random"]
    with LanczosEngine(dtype="c128") as e:
        for spin in (ref.UP, ref.DOWN):
            z, new = e.apply_operator_sum("c", spin, f, L, parts[0], parts[1], src, basis="tj")
            want, wnew = sref.tj_sum("c", spin, L, parts, f, src)
            assert new == wnew and np.max(np.abs(z - want)) <= sref.bound(L, f, src)


# ---- spectral functions -------------------------------------------------------------------------------------------------------------------------
def _reference_records(op, spin, L, parts, gs, f, split):
    """[(type, part, sector, state, weight, sigma)] as spectral_function_weighted documents them, the states built on the CPU"""
    out = []
    for typ in (0, 1):
        o = op if typ else ref.TRANSPOSE_CONJUGATE[op]
        w = f if typ else np.conj(f)
        new = ref.new_sector(o, spin, L, *parts)
        if new is None:
            continue
        s = -1 if typ else 1
        s2 = 1.0 if o in ref.FERMIONIC else float(s)
        if split and np.any(w.imag):
            pieces = [(p, x) for p, x in (("re", w.real), ("im", w.imag)) if np.any(x)]
        else:
            pieces = [(None, w if np.any(w.imag) else w.real)]
        for part, x in pieces:
            state, _ = sref.hubbard_sum(o, spin, L, parts, x, gs)
            out.append((typ, part, new, state, s2 * np.vdot(state, state).real, float(-s)))
    return out


@pytest.mark.parametrize("parts", [(4, 4), (4, 3)])
@pytest.mark.parametrize("op,spin", [("c", ref.UP), ("c", ref.DOWN), ("n", ref.UP), ("sz", ref.UP)])
def test_spectral_function_k(parts, op, spin):
    """8-site ring, U = 4, q = 0, pi/2, pi: per record the weight to 1e-12, a / b to 1e-8 against the oracle's decomposition started from the state
    built on the CPU, the same step count; f64 records of a complex weight vector carry part = "re" / "im"; the c128 engine on the same model gives
    one record per type whose continued fraction is the sum of the f64 parts' to 1e-8 at eta = 0.1 on 21 frequencies (chosen off the record's
    spectral support, see below: measured 1.6e-4 of max|G| inside the band at omega = 8, where the three truncated fractions are not converged,
    and 1e-15 where they are)"""
    L = 8
    hop, U = _ring(L), np.full(L, 4.0)
    pos = np.arange(L)
    # the c128 engine keeps the f64 engine's ground state itself: one Lanczos step from it, the Ritz vector of a one-dimensional Krylov space
    with LanczosEngine() as e, LanczosEngine(dtype="c128", max_steps=1, min_steps=1) as ec:
        e.assemble_hubbard(L, parts[0], parts[1], hop, U)
        e.keep_states(1)
        eg, zg, _ = e.lanczos(1, want_vectors=True)
        gs = zg[0]
        ec.assemble_hubbard(L, parts[0], parts[1], hop, U)
        ec.keep_states(1)
        ec.lanczos(1, init=gs.astype(np.complex128), want_vectors=False)
        assert np.max(np.abs(ec.state(0) - gs)) <= 1e-14
        for q in (0.0, np.pi / 2, np.pi):
            f = sref.momentum_weights(L, {0.0: 0, np.pi / 2: 2, np.pi: 4}[q])  # the reference's own weights, residues of sin(pi r) and all
            if q != np.pi / 2:
                f = f.real + 0j  # a real weight vector: the public entry point must see that by itself
            recs = e.spectral_function_k(op, q, pos, spin=spin)
            want = _reference_records(op, spin, L, parts, gs, f, True)
            assert [(r["type"], r["part"]) for r in recs] == [(t, p) for t, p, _, _, _, _ in want], (op, q)
            if q == np.pi / 2:
                assert {r["part"] for r in recs} == {"re", "im"}
            else:  # commensurate momenta: no record of a part made of rounding residues
                assert all(r["part"] is None for r in recs) and len(recs) == len({r["type"] for r in recs})
            for r, (typ, part, new, state, ws2, msign) in zip(recs, want):
                assert r["sector"] == new and r["sigma"] == msign and r["Eg"] == eg[0]
                # S^z_{q=0} in the (4, 4) sector: every element of the state is within its rounding bound of 0 (the engine gives exactly 0 and no
                # decomposition; the site loop on the CPU may leave rounding noise): there is nothing to decompose on either side
                zero = len(state) * sref.bound(L, f, gs) ** 2
                if abs(ws2) <= zero:
                    assert abs(r["weight"]) <= zero and (r["steps"] == 0) == (r["weight"] == 0.0)
                    continue
                print("%s spin %d q %.3f type %d part %s: weight %.3e" % (op, spin, q, typ, part, abs(r["weight"] - ws2) / abs(ws2)))
                assert abs(r["weight"] - ws2) <= 1e-12 * abs(ws2), (op, q, typ, part, r["weight"], ws2)
                A = oracle.hubbard_csr(L, new[0], new[1], hop, U)
                steps, ao, bo, _, _ = oracle.lanczos_decomposition(A, state)
                print("    steps %d / %d a %.3e b %.3e" % (r["steps"], steps, rel(r["a"], ao) if r["steps"] == steps else -1, rel(r["b"], bo) if r["steps"] == steps else -1))
                assert r["steps"] == steps and rel(r["a"], ao) < 1e-8 and rel(r["b"], bo) < 1e-8, (op, q, typ, part)
            recs_c = ec.spectral_function_k(op, q, pos, spin=spin, energy=eg[0])
            assert all(r["part"] is None for r in recs_c) and [r["type"] for r in recs_c] == sorted({r["type"] for r in recs})
            for rc in recs_c:
                # G = G_CC + G_SS is an identity of the exact resolvents.  The three decompositions stop where the solver's criterion stops them (the
                # lowest Ritz value to 1e-12), in three different Krylov spaces, so inside the band the truncated fractions differ by their truncation
                # errors (test_spectral_function measures 2 - 5 % of max|G| against the Lehmann sum at this eta).  The 21 frequencies are therefore
                # taken on the side of the axis that holds none of the record's poles, 0.5 or more away from the spectrum of sigma (H - Eg), where
                # an n-step fraction converges geometrically in n and all three are converged to rounding: the test is of the split, not of the solver.
                omega = rc["sigma"] * np.linspace(0.5, 8.5, 21) + 0.1j  # (the poles of a record are at omega = -sigma (E_n - Eg))
                w_parts = sum(r["weight"] for r in recs if r["type"] == rc["type"])
                assert abs(rc["weight"] - w_parts) <= 1e-12 * abs(w_parts) or w_parts == rc["weight"] == 0.0, (op, q, rc["type"])  # <phi|phi> = <C|C> + <S|S>
                g_parts = sum(continued_fraction(r, omega) for r in recs if r["type"] == rc["type"])
                g_c = continued_fraction(rc, omega)
                scale = np.max(np.abs(g_parts))
                if scale == 0.0:
                    assert np.all(g_c == 0)
                    continue
                print("    c128 type %d: %.3e" % (rc["type"], np.max(np.abs(g_c - g_parts)) / scale))
                assert np.max(np.abs(g_c - g_parts)) <= 1e-8 * scale, (op, q, rc["type"])


def test_sum_rules():
    """sum_q <c_q^+ c_q> over the chain momenta is N_spin; <n_q=0 n_q=0> = N^2 / L; Heisenberg: <sz_q=0 sz_q=0> = (L - 2m)^2 / L"""
    L, parts = 8, (4, 3)
    pos = np.arange(L)
    with LanczosEngine() as e:
        e.assemble_hubbard(L, parts[0], parts[1], _ring(L), np.full(L, 4.0))
        e.keep_states(1)
        e.lanczos(1, want_vectors=False)
        for spin in (ref.UP, ref.DOWN):
            total = sum(e.weighted_norm2("c", geometry.momentum_weights(pos, 2 * np.pi * m / L), spin=spin) for m in range(L))
            assert abs(total - parts[spin]) <= 1e-10, (spin, total)
        n0 = e.weighted_norm2("n", geometry.momentum_weights(pos, 0.0), spin=ref.UP)
        assert abs(n0 - parts[0] ** 2 / L) <= 1e-10
        both = np.ones(L) / np.sqrt(L)
        z_up, _ = e.apply_operator_sum("n", ref.UP, both, L, parts[0], parts[1], e.state(0))
        z_all, _ = e.apply_operator_sum("n", ref.DOWN, both, L, parts[0], parts[1], e.state(0), out=z_up)
        assert abs(z_all @ z_all - (parts[0] + parts[1]) ** 2 / L) <= 1e-10  # N^2 / L with N = N_up + N_down
        assert e.weighted_norm2("cdagger", both, spin=ref.UP) > 0
    Lh, m = 12, 5
    with LanczosEngine() as e:
        e.assemble_heisenberg(Lh, m, chain(Lh, 1.0, True), chain(Lh, 1.0, True))
        e.keep_states(1)
        e.lanczos(1, want_vectors=False)
        s0 = e.weighted_norm2("sz", geometry.momentum_weights(np.arange(Lh), 0.0))
        assert abs(s0 - (Lh - 2 * m) ** 2 / Lh) <= 1e-10, s0


# ---- the lanczos driver: -g <op> -k <m>, -w <file> -------------------------------------------------------------------------------------------------
def _parse_comb(text):
    labels = re.search(r"^#INDEXTOCF (.*)$", text, re.M).group(1).split()
    recs = []
    for block in re.split(r"^#ContinuedFraction=\d+\n", text, flags=re.M)[1:]:
        vec = {}
        for name in ("Avector", "Bvector"):
            toks = re.search(r"^#%s (.*)$" % name, block, re.M).group(1).split()
            assert int(toks[0]) == len(toks) - 1
            vec[name] = np.array([float(x) for x in toks[1:]])
        sc = {k: float(v) for k, v in re.findall(r"^#CF(Energy|Weight|Isign)=(\S+)$", block, re.M)}
        recs.append(dict(a=vec["Avector"], b=vec["Bvector"], Eg=sc["Energy"], weight=sc["Weight"], sigma=sc["Isign"]))
    assert len(recs) == len(labels)
    return labels, recs


def test_driver_momentum(tmp_path):
    """lanczos -g c -k 1 on the 6-site ring writes <input basename>0.comb with the records of spectral_function_k at q = 2 pi / 6 (a real engine: four
    records, two parts per type); -w with the same weights in a file gives the same file; -k without -g is an error.  SpectralSteps=12 on both
    sides: the sector of the records has 225 states, about 38 per momentum, and a cosine-weighted state spans two momenta -- 12 steps stay far from
    exhausting that space, where the recurrence amplifies the 1e-7 by which two converged ground states differ."""
    assert os.path.exists(DRIVER), "run __graft_entry__.build()"
    src = os.path.join(GOLD, "hubbard_ring_L6.inp")
    inp = tmp_path / "ring.inp"
    inp.write_text(open(src).read().rstrip("\n") + "\nSpectralSteps=12\n")
    res = subprocess.run([DRIVER, "-f", str(inp), "-g", "c", "-k", "1", "-p", "14"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    comb = tmp_path / "ring.inp0.comb"
    assert comb.exists(), os.listdir(str(tmp_path))
    text = comb.read_text()
    assert text.startswith("Momentum=1\n")
    labels, recs = _parse_comb(text)
    data = geometry.parse_input(open(src).read())
    L, nup, ndown = int(data["TotalNumberOfSites"]), int(data["TargetElectronsUp"]), int(data["TargetElectronsDown"])
    with LanczosEngine() as e:
        e.assemble_hubbard(L, nup, ndown, geometry.terms_from_input(data)[0], data["hubbardU"], data["potentialV"])
        e.keep_states(1)
        e.lanczos(1, init=oracle.fill_random(e.rows(), 1234), want_vectors=False)  # the vector the C++ shim starts from
        want = e.spectral_function_k("c", 2 * np.pi / L, np.arange(L), max_steps=12)
    assert labels == [w["label"] for w in want] == ["0,0,0,0,re", "0,0,0,0,im", "0,1,0,0,re", "0,1,0,0,im"]
    z = np.array([-1.0 + 0.1j, 0.5 + 0.1j, 2.0 + 0.1j])
    for r, w in zip(recs, want):
        assert len(r["a"]) == len(r["b"]) == w["steps"] == 12
        assert rel(r["a"], w["a"]) < 1e-8 and rel(r["b"], w["b"]) < 1e-8
        assert abs(r["weight"] - w["weight"]) <= 1e-8 * abs(w["weight"]) and r["sigma"] == w["sigma"]
        assert abs(r["Eg"] - w["Eg"]) <= 1e-8 * abs(w["Eg"])
        assert np.max(np.abs(continued_fraction(r, z) - continued_fraction(w, z))) <= 1e-8 * np.max(np.abs(continued_fraction(w, z)))
    # the commensurate momentum m = L / 2: real weights, one record per type, none made of rounding residues
    res = subprocess.run([DRIVER, "-f", str(inp), "-g", "c", "-k", str(L // 2), "-p", "14"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert res.returncode == 0 and "modifVector==0" not in res.stderr, res.stderr
    labels_pi, recs_pi = _parse_comb(comb.read_text())
    assert labels_pi == ["0,0,0,0", "0,1,0,0"]
    with LanczosEngine() as e:
        e.assemble_hubbard(L, nup, ndown, geometry.terms_from_input(data)[0], data["hubbardU"], data["potentialV"])
        e.keep_states(1)
        e.lanczos(1, init=oracle.fill_random(e.rows(), 1234), want_vectors=False)
        want_pi = e.spectral_function_k("c", np.pi, np.arange(L), max_steps=12)
    assert [w["label"] for w in want_pi] == labels_pi
    for r, w in zip(recs_pi, want_pi):
        assert len(r["a"]) == w["steps"] and rel(r["a"], w["a"]) < 1e-8 and rel(r["b"], w["b"]) < 1e-8 and abs(r["weight"] - w["weight"]) <= 1e-8 * abs(w["weight"])
    res = subprocess.run([DRIVER, "-f", str(inp), "-g", "c", "-k", "1", "-p", "14"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    wfile = tmp_path / "weights.txt"
    wfile.write_text("".join("%.17g %.17g\n" % (x.real, x.imag) for x in sref.momentum_weights(L, 1)))
    res = subprocess.run([DRIVER, "-f", str(inp), "-g", "c", "-w", str(wfile), "-p", "14"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    labels2, recs2 = _parse_comb(comb.read_text())
    assert labels2 == labels
    for r, r2 in zip(recs, recs2):
        assert len(r2["a"]) == len(r["a"]) and rel(r2["a"], r["a"]) < 1e-8 and rel(r2["b"], r["b"]) < 1e-8 and abs(r2["weight"] - r["weight"]) <= 1e-8 * abs(r["weight"])
    res = subprocess.run([DRIVER, "-f", str(inp), "-k", "1"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert res.returncode == 2 and "-g" in res.stderr


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_statuses(monkeypatch):
    L, nup, ndown = 8, 4, 4
    src = oracle.fill_random(4900, 3)
    lib = _capi.lib()
    one = np.ones(L)

    def vp(a):
        return a.ctypes.data_as(C.c_void_p)

    with LanczosEngine() as e:
        z = np.full(4900, 7.0)
        has, n = C.c_int32(), C.c_int64()
        wi = np.full(L, 0.5)
        # complex weights on an f64 engine, through the C entry: LPP_ERR_INVALID, the destination untouched
        st = lib.lpp_engine_apply_operator_sum_host(e._h, _capi.LPP_OP_N, 0, L, nup, ndown, L, vp(one), vp(wi), vp(src), vp(z), 0, C.byref(has), C.byref(n))
        assert st == _capi.LPP_ERR_INVALID and np.all(z == 7.0)
        with pytest.raises(LppError) as ei:
            e.apply_operator_sum("n", 0, one + 0.5j, L, nup, ndown, src)
        assert ei.value.status == _capi.LPP_ERR_INVALID
        # wrong weight count
        st = lib.lpp_engine_apply_operator_sum_host(e._h, _capi.LPP_OP_N, 0, L, nup, ndown, L - 1, vp(one), None, vp(src), vp(z), 0, C.byref(has), C.byref(n))
        assert st == _capi.LPP_ERR_INVALID and np.all(z == 7.0)
        with pytest.raises(LppError):
            e.apply_operator_sum("c", 0, np.ones(L + 1), L, nup, ndown, src)
        with pytest.raises(LppError):
            e.bench_operator_sum("c", 0, np.ones(L - 1), L, nup, ndown)
        # no sector
        assert e.apply_operator_sum("cdagger", ref.UP, one, L, L, 3, oracle.fill_random(ref.comb(L, 3), 1)) == (None, None)
        with pytest.raises(ValueError):
            e.apply_operator_sum("nil", 0, one, L, nup, ndown, src)
        with pytest.raises(LppError):
            e.apply_operator_sum("c", 2, one, L, nup, ndown, src)  # bad spin
        with pytest.raises(LppError):
            e.weighted_norm2("c", one)  # no model, no resident state
    # a hole-major t-J engine where apply_operator refuses
    Lt = 12
    hop = _ring(Lt)
    monkeypatch.setenv("LPP_TJ_LAYOUT", "1")
    with LanczosEngine() as e:
        e.assemble_tj(Lt, 4, 4, hop, 0.5 * np.abs(hop), 0.5 * np.abs(hop), np.zeros((Lt, Lt)))
        assert e.layout()["kernel"] == 5
        with pytest.raises(LppError) as ei:
            e.apply_operator_sum("n", 0, one, L, nup, ndown, src)
        assert ei.value.status == _capi.LPP_ERR_STATE


def test_multi_rank_engine_is_refused():
    """two ranks as threads of one process (ThreadComm): every operator-sum entry point answers LPP_ERR_STATE and launches nothing"""
    from lanczosplusplus_amd.comm import ThreadComm, ThreadGroup
    world, L, nup, ndown = 2, 8, 4, 4
    n_up = n_dn = 70
    per = -(-n_dn // world)
    chunk = _capi.lib().lpp_xchg_chunk(n_up, n_dn, world)
    dev = torch.device("cuda", 0)
    group = ThreadGroup(world, dev)
    out = [None] * world
    hop, U = _ring(L), np.full(L, 4.0)

    def run(rank):
        try:
            torch.cuda.set_device(dev)
            comm = ThreadComm(group, rank, per * n_up, 50, False, xchg_chunk=chunk)
            with comm.stream_context():
                e = LanczosEngine(max_steps=50, save_vectors=0, stream=comm.stream_handle)
                e.assemble_hubbard(L, nup, ndown, hop, U, comm=comm)
                got = []
                for call in (lambda: e.apply_operator_sum("c", 0, np.ones(L), L, nup, ndown, np.zeros(4900)),
                             lambda: e.bench_operator_sum("c", 0, np.ones(L), L, nup, ndown)):
                    try:
                        call()
                        got.append(None)
                    except LppError as err:
                        got.append(err.status)
                # the device-vector apply, the norm and the decomposition through the C entries (the Python methods ask for a model first)
                lib, one = _capi.lib(), np.ones(L)
                p = one.ctypes.data_as(C.c_void_p)
                v, has, n = C.c_double(), C.c_int32(), C.c_int32()
                buf = np.zeros(16)
                bp = buf.ctypes.data_as(C.c_void_p)
                got.append(lib.lpp_engine_apply_operator_sum(e._h, _capi.LPP_OP_C, 0, L, nup, ndown, L, p, None, bp, bp, 0, C.byref(has)))
                got.append(lib.lpp_engine_sum_norm2(e._h, 0, _capi.LPP_OP_C, 0, L, nup, ndown, L, p, None, C.byref(v), C.byref(has)))
                got.append(lib.lpp_engine_spectral_decomposition_sum(e._h, 0, e._h, _capi.LPP_OP_C, 0, L, nup, ndown, L, p, None, C.byref(v), C.byref(n), bp, bp, None))
                e.close()
            out[rank] = got
        except Exception:
            import traceback
            out[rank] = traceback.format_exc()
            try:
                group.barrier.abort()
            except Exception:
                pass

    threads = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a rank is stuck inside a collective"
    assert out == [[_capi.LPP_ERR_STATE] * 5] * world, out
