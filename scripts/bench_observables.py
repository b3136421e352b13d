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
Usage: hipcc --offload-arch=gfx950 -O3 -o scripts/calib_stream scripts/calib_stream.hip
       python scripts/bench_observables.py [--lx 4 --ly 4 --nup 8 --ndown 8] [--calib-stream scripts/calib_stream] [--spectral-steps 40]"""
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


def stream_rate(exe):
    """GB/s of calib_stream's CALIB_LINE line, measured now in a child process"""
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if res.returncode != 0:
        raise SystemExit("calib_stream failed (%d): %s" % (res.returncode, res.stderr))
    m = re.search(r"^%s\s+\S+ ms\s+(\S+) GB/s$" % CALIB_LINE, res.stdout, re.M)
    if not m:
        raise SystemExit("calib_stream printed no %s line:\n%s" % (CALIB_LINE, res.stdout))
    return float(m.group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lx", type=int, default=4)
    ap.add_argument("--ly", type=int, default=4)
    ap.add_argument("--nup", type=int, default=8)
    ap.add_argument("--ndown", type=int, default=8)
    ap.add_argument("--calib-stream", default="", help="path of the calib_stream binary; empty: no ratio")
    ap.add_argument("--spectral-steps", type=int, default=40)
    ap.add_argument("--gs-steps", type=int, default=200)
    a = ap.parse_args()
    L = a.lx * a.ly
    hop, U = square(a.lx, a.ly, -1.0), np.full(L, 4.0)
    rate = stream_rate(a.calib_stream) if a.calib_stream else 0.0
    out = dict(config="%dx%d %dup %ddown U=4" % (a.lx, a.ly, a.nup, a.ndown),
               stream_rate=dict(tool="scripts/calib_stream.hip", line=CALIB_LINE, kind="read, 16 bytes per lane, 4 GiB", gbs=rate) if rate else None)
    with LanczosEngine(max_steps=a.gs_steps, save_vectors=0) as e:
        ops = {}
        for name, (op, spin) in (("c_up", ("c", 0)), ("c_down", ("c", 1)), ("splus", ("splus", 0))):
            ms, by = e.bench_operator(op, L // 2, spin, L, a.nup, a.ndown, warmup=2, iters=10)
            gbs = by / ms * 1e-6
            ops[name] = dict(ms=round(ms, 4), model_bytes=by, gbs=round(gbs, 1), ratio_to_stream=round(gbs / rate, 3) if rate else None)
        out["operator"] = ops
        t0 = time.time()
        e.assemble_hubbard(L, a.nup, a.ndown, hop, U)
        out["assemble_s"] = round(time.time() - t0, 3)
        out["states"] = e.rows()
        e.keep_states(1)
        t0 = time.time()
        eg, _, st = e.lanczos(1, want_vectors=False)
        out["ground_state"] = dict(E0=eg[0], steps=st["steps"], seconds=round(time.time() - t0, 3))
        t0 = time.time()
        res, tr = e.two_point("c", (0, 0))
        out["two_point_c_up"] = dict(seconds=round(time.time() - t0, 3), trace=float(tr))
        t0 = time.time()
        recs = []
        for site in range(L):
            recs += e.spectral_function("c", site, site, 0, max_steps=a.spectral_steps, eps=0.0)
        out["density_of_states"] = dict(sites=L, decompositions=len(recs), seconds=round(time.time() - t0, 3), assemblies=e.sector_assemblies,
                                        spectral_steps=a.spectral_steps, weight_sum_site0=recs[0]["weight"] + recs[1]["weight"])
        # the same kernels: a spectral decomposition and the ground-state solve of the SAME sector engine
        sector = recs[0]["sector"]
        eng = e._sectors[sector]
        rec = e.spectral_function("c", 0, 0, 0, max_steps=a.spectral_steps, eps=0.0)[0]
        eng.set_solver(max_steps=a.spectral_steps, min_steps=4, eps=0.0, reortho=False, save_vectors=0)
        _, _, sg = eng.lanczos(1, want_vectors=False)
        gs_ms = 1e3 * sg["seconds_total"] / max(sg["steps_enqueued"], 1)
        out["step_time"] = dict(sector=list(sector), spectral_ms_per_step=round(rec["ms_per_step"], 4), ground_state_ms_per_step=round(gs_ms, 4),
                                ratio=round(rec["ms_per_step"] / gs_ms, 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
