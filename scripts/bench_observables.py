#!/usr/bin/env python
"""Measure the observables path at BASELINE config 2 (4x4 Hubbard, 8 up 8 down, U = 4, 1.66e8 states) and print ONE JSON line
(committed as profiles/observables_c2.json):
  operator kernel   ms and GB/s of c up, c down, splus against the byte model 8 * (N_dst read + write + source entries read) and, with
                    --calib-stream (the binary built from scripts/calib_stream.hip, run here as a child process before this process opens
                    the GPU), the ratio to the rate of its `stream16` line.  calib_stream measures READ rates of a 4 GiB buffer (16 bytes per
                    lane), it has no copy kernel: the JSON says which line was used and that it is a read rate.
  two_point(c, up)  total seconds
  density of states 16 sites, spin up: total seconds, sector assemblies
  step time         ms_per_step of a spectral decomposition next to the ground-state solve of the same sector's engine
--model tj: the same figures for the one-orbital t-J model (c128, t = -1, J = 0.4, W = -0.1 as bench.py's t-J workloads; committed for BASELINE
config 4 -- --lx 5 --ly 4 --nup 9 --ndown 9 -- as profiles/observables_tj_c4.json), the operator kernel being k_obs_apply_tj, plus
  hubbard_yardstick k_obs_apply's c up in the same process and dtype on the Hubbard sector L = 14 (7, 6): 1.03e7 states, about config 4's
                    vector bytes.
A vector of config 4 (148 MB) fits the MI355X's 256 MB Infinity Cache while calib_stream reads 4 GiB from HBM: the stream yardstick is flattered.
--model heisenberg --sites L --m M: the S = 1/2 Heisenberg chain (f64, J = 1, open ends as BASELINE config 3; committed for (28;14) and (32;16) as
profiles/observables_heis_L28.json / _L32.json), the operator kernel being k_obs_apply_heis:
  operator          splus at site 0 (a gather inside the runs of equal high part), splus at site L-1 (run onto run), sz at site 0 and at site L-1
  hubbard_yardstick k_obs_apply's c up on config 2 (16 sites, 8 up 8 down) in the same process, and `bar`: every launch's share of the stream rate
                    against half of the share that yardstick gets
  unless --operators-only: two_point(sz), two_point(splus), the -g sz set of one centre site (L pairs) and the step times as above
--model heisenberg --twice-s T --sites L --m M (T > 1): the spin-S chain in the opt-in digit basis (f64; committed for S = 1, (18;18), as
profiles/observables_heis_spin1_L18.json), the operator kernel being k_obs_apply_heis_spin:
  operator          splus and sz at site 0 and at site L-1, accumulating launches, and each one's ratio to the SAME-SITE launch of
  spin_half_yardstick   k_obs_apply_heis at (28;14) in the same process (4.0e7 states), next to hubbard_yardstick and `bar` as above
  unless --operators-only: the ring (J = 1, periodic): two_point("sz", basis="spin") and one S^zz(q = pi, w) decomposition (spectral_function_k)
Usage: hipcc --offload-arch=gfx950 -O3 -o scripts/calib_stream scripts/calib_stream.hip
       python scripts/bench_observables.py [--model hubbard|tj] [--lx 4 --ly 4 --nup 8 --ndown 8] [--calib-stream scripts/calib_stream] [--spectral-steps 40]
       python scripts/bench_observables.py --model heisenberg --sites 28 --m 14 [--operators-only] [--calib-stream scripts/calib_stream]
       python scripts/bench_observables.py --model heisenberg --twice-s 2 --sites 18 --m 18 --operators-only"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lanczosplusplus_amd import LanczosEngine  # noqa: E402


def square(lx, ly, v):
    L = lx * ly
    m = np.zeros((L, L))
    for x in range(lx):
        for y in range(ly):
            s = x * ly + y
            for (xx, yy) in (((x + 1) % lx, y), (x, (y + 1) % ly)):
                t = xx * ly + yy
                if t != s:
                    m[s, t] = m[t, s] = v
    return m


CALIB_LINE = "stream16"
YARD = (14, 7, 6)  # the Hubbard sector of --model tj's yardstick: 1.03e7 states, about config 4's vector bytes


def stream_rate(exe):
    """GB/s of calib_stream's CALIB_LINE line, measured now in a child process"""
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if res.returncode != 0:
        raise SystemExit("calib_stream failed (%d): %s" % (res.returncode, res.stderr))
    m = re.search(r"^%s\s+\S+ ms\s+(\S+) GB/s$" % CALIB_LINE, res.stdout, re.M)
    if not m:
        raise SystemExit("calib_stream printed no %s line:\n%s" % (CALIB_LINE, res.stdout))
    return float(m.group(1))


def chain(L, v):
    m = np.zeros((L, L))
    for i in range(L - 1):
        m[i, i + 1] = m[i + 1, i] = v
    return m


def heisenberg(a, rate):
    """--model heisenberg: one JSON line"""
    L, m = a.sites, a.m
    out = dict(config="Heisenberg S=1/2 chain L=%d szPlusConst=%d J=1 open f64" % (L, m),
               stream_rate=dict(tool="scripts/calib_stream.hip", line=CALIB_LINE, kind="read, 16 bytes per lane, 4 GiB", gbs=rate) if rate else None)
    with LanczosEngine(max_steps=a.gs_steps, save_vectors=0) as e:

        def bench(op, site, spin, sites, nup, ndown, basis):
            ms, by = e.bench_operator(op, site, spin, sites, nup, ndown, warmup=2, iters=10, basis=basis)
            gbs = by / ms * 1e-6
            return dict(ms=round(ms, 4), model_bytes=by, gbs=round(gbs, 1), ratio_to_stream=round(gbs / rate, 3) if rate else None)

        ops = {}
        for name, (op, site) in (("splus_site0", ("splus", 0)), ("splus_last_site", ("splus", L - 1)), ("sz_site0", ("sz", 0)), ("sz_last_site", ("sz", L - 1))):
            ops[name] = bench(op, site, 0, L, m, 0, "spin_half")
        out["operator"] = ops
        yard = bench("c", 8, 0, 16, 8, 8, "hubbard")
        yard["sector"] = [16, 8, 8]
        out["hubbard_yardstick_c_up"] = yard
        worst = min(ops, key=lambda k: ops[k]["gbs"])
        out["bar"] = dict(rule="every launch >= half of the Hubbard c up launch's share of the stream rate (same run)", worst=worst,
                          worst_over_yardstick=round(ops[worst]["gbs"] / yard["gbs"], 3), met=bool(ops[worst]["gbs"] >= 0.5 * yard["gbs"]))
        if a.operators_only:
            print(json.dumps(out))
            return
        j = chain(L, 1.0)
        t0 = time.time()
        e.assemble_heisenberg(L, m, j, j)
        out["assemble_s"] = round(time.time() - t0, 3)
        out["layout_kernel"] = e.layout()["kernel"]
        out["states"] = e.rows()
        e.keep_states(1)
        t0 = time.time()
        eg, _, st = e.lanczos(1, want_vectors=False)
        out["ground_state"] = dict(E0=eg[0], steps=st["steps"], seconds=round(time.time() - t0, 3))
        for op in ("sz", "splus"):
            t0 = time.time()
            res, tr = e.two_point(op, (0, 0))
            out["two_point_" + op] = dict(seconds=round(time.time() - t0, 3), trace=float(tr))
        t0 = time.time()
        recs = []
        for site in range(L):
            recs += e.spectral_function("sz", L // 2, site, 0, max_steps=a.spectral_steps, eps=0.0)
        out["spectral_sz_centre_set"] = dict(pairs=L, decompositions=len(recs), seconds=round(time.time() - t0, 3), assemblies=e.sector_assemblies,
                                             spectral_steps=a.spectral_steps, note="-g sz decomposes the raw 1 - 2 bit = -2 S^z")
        again = e.spectral_function("sz", 0, 0, 0, max_steps=a.spectral_steps, eps=0.0)
        eng = e._sectors[again[0]["sector"]]
        eng.set_solver(max_steps=a.spectral_steps, min_steps=4, eps=0.0, reortho=False, save_vectors=0)
        _, _, sg = eng.lanczos(1, want_vectors=False)
        gs_ms = 1e3 * sg["seconds_total"] / max(sg["steps_enqueued"], 1)
        out["step_time"] = dict(sector=list(again[0]["sector"]), states=eng.rows(), layout_kernel=eng.layout()["kernel"], spectral_ms_per_step=round(again[0]["ms_per_step"], 4),
                                ground_state_ms_per_step=round(gs_ms, 4), ratio=round(again[0]["ms_per_step"] / gs_ms, 4))
    print(json.dumps(out))


SPIN_HALF_YARD = (28, 14)  # the S = 1/2 sector of --twice-s's yardstick: 4.0e7 states


def heisenberg_spin(a, rate):
    """--model heisenberg --twice-s T: one JSON line"""
    L, m, t = a.sites, a.m, a.twice_s
    out = dict(config="Heisenberg twiceS=%d chain L=%d szPlusConst=%d J=1 f64, digit basis" % (t, L, m),
               stream_rate=dict(tool="scripts/calib_stream.hip", line=CALIB_LINE, kind="read, 16 bytes per lane, 4 GiB", gbs=rate) if rate else None)
    with LanczosEngine(max_steps=a.gs_steps, save_vectors=0) as e:

        def bench(op, site, sites, nup, ndown, basis, twiceS=None):
            ms, by = e.bench_operator(op, site, 0, sites, nup, ndown, warmup=2, iters=10, basis=basis, twiceS=twiceS)
            gbs = by / ms * 1e-6
            return dict(ms=round(ms, 4), model_bytes=by, gbs=round(gbs, 1), ratio_to_stream=round(gbs / rate, 3) if rate else None)

        ops, half = {}, {}
        Lh, mh = SPIN_HALF_YARD
        for name, op, last in (("splus_site0", "splus", False), ("splus_last_site", "splus", True), ("sz_site0", "sz", False), ("sz_last_site", "sz", True)):
            ops[name] = bench(op, L - 1 if last else 0, L, m, 0, "spin", t)
            half[name] = bench(op, Lh - 1 if last else 0, Lh, mh, 0, "spin_half")
            ops[name]["ms_over_spin_half_same_site"] = round(ops[name]["ms"] / half[name]["ms"], 3)
            ops[name]["gbs_over_spin_half_same_site"] = round(ops[name]["gbs"] / half[name]["gbs"], 3)
        out["operator"] = ops
        half["sector"] = list(SPIN_HALF_YARD)
        out["spin_half_yardstick"] = half
        yard = bench("c", 8, 16, 8, 8, "hubbard")
        yard["sector"] = [16, 8, 8]
        out["hubbard_yardstick_c_up"] = yard
        worst = min(ops, key=lambda k: ops[k]["gbs"])
        out["bar"] = dict(rule="every launch >= half of the Hubbard c up launch's share of the stream rate (same run)", worst=worst,
                          worst_over_yardstick=round(ops[worst]["gbs"] / yard["gbs"], 3), met=bool(ops[worst]["gbs"] >= 0.5 * yard["gbs"]))
        if a.operators_only:
            print(json.dumps(out))
            return
        j = chain(L, 1.0)
        j[0, L - 1] = j[L - 1, 0] = 1.0
        t0 = time.time()
        e.assemble_heisenberg(L, m, j, j, twiceS=t)
        out["assemble_s"] = round(time.time() - t0, 3)
        out["layout_kernel"] = e.layout()["kernel"]
        out["states"] = e.rows()
        e.keep_states(1)
        t0 = time.time()
        eg, _, st = e.lanczos(1, want_vectors=False)
        out["ground_state"] = dict(E0=eg[0], steps=st["steps"], seconds=round(time.time() - t0, 3))
        t0 = time.time()
        res, tr = e.two_point("sz", basis="spin")
        out["two_point_sz"] = dict(seconds=round(time.time() - t0, 3), trace=float(tr), nearest_neighbour=float(res[0, 1]))
        t0 = time.time()
        recs = e.spectral_function_k("sz", np.pi, np.arange(L), max_steps=a.spectral_steps, eps=0.0, basis="spin")
        out["szz_q_pi"] = dict(seconds_both_types=round(time.time() - t0, 3), records=len(recs), steps=[r["steps"] for r in recs], assemblies=e.sector_assemblies,
                               ms_per_step=[round(r["ms_per_step"], 4) for r in recs], static_structure_factor=float(recs[0]["modif_norm2"]),
                               note="the first record includes the assembly of the sector engine")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lx", type=int, default=4)
    ap.add_argument("--ly", type=int, default=4)
    ap.add_argument("--nup", type=int, default=8)
    ap.add_argument("--ndown", type=int, default=8)
    ap.add_argument("--calib-stream", default="", help="path of the calib_stream binary; empty: no ratio")
    ap.add_argument("--spectral-steps", type=int, default=40)
    ap.add_argument("--gs-steps", type=int, default=200)
    ap.add_argument("--model", choices=("hubbard", "tj", "heisenberg"), default="hubbard")
    ap.add_argument("--sites", type=int, default=28, help="--model heisenberg: chain length")
    ap.add_argument("--m", type=int, default=14, help="--model heisenberg: szPlusConst")
    ap.add_argument("--twice-s", type=int, default=1, help="--model heisenberg: twiceS; above 1 the opt-in digit basis (k_obs_apply_heis_spin) is measured")
    ap.add_argument("--operators-only", action="store_true", help="--model heisenberg: the operator launches and the yardstick only (no matrix)")
    a = ap.parse_args()
    L = a.lx * a.ly
    tj = a.model == "tj"
    hop, U = square(a.lx, a.ly, -1.0), np.full(L, 4.0)
    rate = stream_rate(a.calib_stream) if a.calib_stream else 0.0
    if a.model == "heisenberg":
        return heisenberg_spin(a, rate) if a.twice_s > 1 else heisenberg(a, rate)
    out = dict(config=("t-J %dx%d %dup %ddown t=-1 J=0.4 W=-0.1 c128" if tj else "%dx%d %dup %ddown U=4") % (a.lx, a.ly, a.nup, a.ndown),
               stream_rate=dict(tool="scripts/calib_stream.hip", line=CALIB_LINE, kind="read, 16 bytes per lane, 4 GiB", gbs=rate) if rate else None)
    basis = "tj" if tj else "hubbard"
    with LanczosEngine(dtype="c128" if tj else "f64", max_steps=a.gs_steps, save_vectors=0) as e:

        def bench(op, site, spin, sites, nup, ndown, basis):
            ms, by = e.bench_operator(op, site, spin, sites, nup, ndown, warmup=2, iters=10, basis=basis)
            gbs = by / ms * 1e-6
            return dict(ms=round(ms, 4), model_bytes=by, gbs=round(gbs, 1), ratio_to_stream=round(gbs / rate, 3) if rate else None)

        ops = {}
        for name, (op, spin) in (("c_up", ("c", 0)), ("c_down", ("c", 1)), ("splus", ("splus", 0))):
            ops[name] = bench(op, L // 2, spin, L, a.nup, a.ndown, basis)
        out["operator"] = ops
        if tj:
            yard = bench("c", YARD[0] // 2, 0, YARD[0], YARD[1], YARD[2], "hubbard")
            yard["sector"] = list(YARD)
            out["hubbard_yardstick_c_up"] = yard
            out["c_up_ratio_to_hubbard_kernel"] = round(ops["c_up"]["gbs"] / yard["gbs"], 3)
            out["note"] = "a 148 MB vector fits the 256 MB Infinity Cache; calib_stream reads 4 GiB from HBM, so ratio_to_stream is flattered"
        t0 = time.time()
        if tj:
            e.assemble_tj(L, a.nup, a.ndown, hop, square(a.lx, a.ly, 0.4), square(a.lx, a.ly, 0.4), square(a.lx, a.ly, -0.1))
            out["layout_kernel"] = e.layout()["kernel"]
        else:
            e.assemble_hubbard(L, a.nup, a.ndown, hop, U)
        out["assemble_s"] = round(time.time() - t0, 3)
        out["states"] = e.rows()
        (e.keep_states_tj if tj else e.keep_states)(1)
        t0 = time.time()
        eg, _, st = e.lanczos(1, want_vectors=False)
        out["ground_state"] = dict(E0=eg[0], steps=st["steps"], seconds=round(time.time() - t0, 3))
        t0 = time.time()
        res, tr = e.two_point("c", (0, 0))
        out["two_point_c_up"] = dict(seconds=round(time.time() - t0, 3), trace=float(np.real(tr)))
        t0 = time.time()
        recs = []
        for site in range(L):
            recs += e.spectral_function("c", site, site, 0, max_steps=a.spectral_steps, eps=0.0)
        out["density_of_states"] = dict(sites=L, decompositions=len(recs), seconds=round(time.time() - t0, 3), assemblies=e.sector_assemblies,
                                        spectral_steps=a.spectral_steps, weight_sum_site0=recs[0]["weight"] + recs[1]["weight"])
        # the same kernels: a spectral decomposition and the ground-state solve of the SAME sector engine
        def step_time(rec):
            eng = e._sectors[rec["sector"]]
            eng.set_solver(max_steps=a.spectral_steps, min_steps=4, eps=0.0, reortho=False, save_vectors=0)
            _, _, sg = eng.lanczos(1, want_vectors=False)
            gs_ms = 1e3 * sg["seconds_total"] / max(sg["steps_enqueued"], 1)
            return dict(sector=list(rec["sector"]), states=eng.rows(), layout_kernel=eng.layout()["kernel"], spectral_ms_per_step=round(rec["ms_per_step"], 4),
                        ground_state_ms_per_step=round(gs_ms, 4), ratio=round(rec["ms_per_step"] / gs_ms, 4))

        again = e.spectral_function("c", 0, 0, 0, max_steps=a.spectral_steps, eps=0.0)
        out["step_time"] = step_time(again[0])
        if tj:  # the N - 1 sector as well: the one a single-hole spectral function runs in
            out["step_time_c_sector"] = step_time(again[1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
