#!/usr/bin/env python
"""Measure the site-weighted operator sums at BASELINE config 2 (4x4 Hubbard, 8 up 8 down, 1.66e8 states) and print ONE JSON line (committed as
profiles/operator_sum_c2.json):
  sum        c up, c down, n, sz with the weights exp(i q.x)/sqrt(L) of the generic q = (0.7, 1.1), all 16 of them non-zero (the f64 engine of config 2 takes their real part, as one part of the
             f64 split does; --dtype c128 takes them whole), each as the ONE fused launch and, on a second engine made under LPP_OBS_SUM_CHAIN=1, as the chain of one-site
             launches: ms, GB/s against the byte model 8|16 * (N_dst written + N_src read once), the ratio chain / fused, and with --calib-stream the
             share of the rate of calib_stream's `stream16` line (a READ rate of a 4 GiB buffer, measured in a child process before this one opens the GPU)
  lds_staged whether a form of k_obs_sum_move that stages the source block in LDS was tried (it was not: see the note in the JSON)
  sweep      with --sweep: the 16 momenta of the 4x4 lattice, A(k,w) of c up -- spectral_function_k, --spectral-steps steps per fraction -- in seconds,
             next to the count of decompositions the pair route needs (L (L + 1) / 2 pairs of up to four types)
Usage: hipcc --offload-arch=gfx950 -O3 -o scripts/calib_stream scripts/calib_stream.hip
       python scripts/bench_operator_sum.py [--calib-stream scripts/calib_stream] [--dtype c128|f64] [--sweep] [--spectral-steps 40]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lanczosplusplus_amd import LanczosEngine, geometry  # noqa: E402

CALIB_LINE = "stream16"
Q = (0.7, 1.1)  # no lattice momentum of any lattice here: all cosines and sines are far from 0


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


def stream_rate(exe):
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
    ap.add_argument("--dtype", choices=("f64", "c128"), default="f64")
    ap.add_argument("--calib-stream", default="", help="path of the calib_stream binary; empty: no ratio")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sweep", action="store_true", help="also time the A(k,w) sweep over all momenta (assembles the model, solves the ground state)")
    ap.add_argument("--spectral-steps", type=int, default=40)
    a = ap.parse_args()
    L = a.lx * a.ly
    rate = stream_rate(a.calib_stream) if a.calib_stream else 0.0
    pos = np.array([[s // a.ly, s % a.ly] for s in range(L)], float)
    # a generic q: every one of the L weights is a weight (at a lattice momentum half of the cosines are 0 and the chain skips those sites)
    w = geometry.momentum_weights(pos, Q)
    if a.dtype == "f64":
        w = w.real.copy()
    cases = (("c_up", "c", 0), ("c_down", "c", 1), ("n_up", "n", 0), ("sz", "sz", 0))
    out = dict(config="%dx%d %dup %ddown %s, weights exp(i q.x)/sqrt(L) at q=(0.7,1.1)%s" % (a.lx, a.ly, a.nup, a.ndown, a.dtype, ", real part" if a.dtype == "f64" else ""),
               stream_rate=dict(tool="scripts/calib_stream.hip", line=CALIB_LINE, kind="read, 16 bytes per lane, 4 GiB", gbs=rate) if rate else None,
               nonzero_weights=int(np.count_nonzero(w)), smallest_weight_over_largest=float(np.min(np.abs(w)) / np.max(np.abs(w))), iters=a.iters)
    res = {}
    for mode in ("fused", "chain"):
        if mode == "chain":
            os.environ["LPP_OBS_SUM_CHAIN"] = "1"  # read when the engine first plans an operator
        else:
            os.environ.pop("LPP_OBS_SUM_CHAIN", None)
        with LanczosEngine(dtype=a.dtype) as e:
            for name, op, spin in cases:
                ms, by = e.bench_operator_sum(op, spin, w, L, a.nup, a.ndown, warmup=2, iters=a.iters)
                gbs = by / ms * 1e-6
                res.setdefault(name, {})[mode] = dict(ms=round(ms, 4), model_bytes=by, model_gbs=round(gbs, 1), ratio_to_stream=round(gbs / rate, 3) if rate else None)
    os.environ.pop("LPP_OBS_SUM_CHAIN", None)
    for name in res:
        res[name]["chain_over_fused"] = round(res[name]["chain"]["ms"] / res[name]["fused"]["ms"], 3)
    out["sum"] = res
    out["fused_not_slower_on_every_line"] = bool(all(v["chain_over_fused"] >= 1.0 for v in res.values()))
    out["lds_staged"] = dict(tried=False, note="k_obs_sum_move gathers from registers through L1 / L2 (the up species' source block is at most 103 KB at 16 sites); "
                                               "no LDS-staged form was built or measured")
    if a.sweep:
        with LanczosEngine(dtype=a.dtype, save_vectors=0) as e:
            t0 = time.time()
            e.assemble_hubbard(L, a.nup, a.ndown, square(a.lx, a.ly, -1.0), np.full(L, 4.0))
            e.keep_states(1)
            eg, _, st = e.lanczos(1, want_vectors=False)
            setup = time.time() - t0
            t0 = time.time()
            recs = []
            for kx in range(a.lx):
                for ky in range(a.ly):
                    recs += e.spectral_function_k("c", [2 * np.pi * kx / a.lx, 2 * np.pi * ky / a.ly], pos, spin=0, max_steps=a.spectral_steps, eps=0.0)
            out["sweep"] = dict(momenta=L, decompositions=len(recs), seconds=round(time.time() - t0, 3), setup_seconds=round(setup, 3), assemblies=e.sector_assemblies,
                                spectral_steps=a.spectral_steps, E0=eg[0], weight_sum=float(sum(r["weight"] for r in recs)),
                                pair_route=dict(pairs=L * (L + 1) // 2, decompositions=L * 2 + (L * (L - 1) // 2) * 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
