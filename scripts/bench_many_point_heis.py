#!/usr/bin/env python
"""Measure the many-point path of the S = 1/2 Heisenberg basis on the open chain of 28 sites (szPlusConst 14, J = 1, 4.0e7 states, f64) on the resident
ground state and write ONE JSON document (committed as profiles/many_point_heis_L28.json).  All in one run:
  (a) a four-spin string  sz 0; sz 1; sz 14; sz 15  and an exchange string  splus 0; sminus 1; splus 14; sminus 15  through
      LanczosEngine.many_point(basis="spin_half") (planning, upload of the run entries, the bracket kernel, the reduction and the sync: a host clock
      around the whole call) against the same string chained through four lpp_engine_apply_operator_heis launches on device vectors plus a dot
      product (host clock around the four enqueues, the engine's sync, torch.dot and torch's sync).  The values are compared before anything is
      timed, and whether their bits match is recorded.
  (b) 8 strings in one launch against 8 launches of one string (device events, lpp_engine_bench_string_dot_heis).
  (c) the bytes of each string of (a) -- bra once, one ket element per destination the string reaches -- over its kernel time (device events), against
      the `stream16` read rate of scripts/calib_stream.hip measured in a child process before this process opens the GPU.
Warm-up: 2 calls of every timed shape; repetition: 10 calls, every time listed, the median quoted.
Usage: hipcc --offload-arch=gfx950 -O3 -o scripts/calib_stream scripts/calib_stream.hip
       python scripts/bench_many_point_heis.py [--calib-stream scripts/calib_stream] [--out profiles/many_point_heis_L28.json] [--sites 28 --m 14]"""
import argparse
import ctypes as C
import json
import os
import struct
import sys
from math import comb

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_many_point import REPEAT, WARMUP, timed  # noqa: E402
from bench_observables import CALIB_LINE, chain, stream_rate  # noqa: E402
from lanczosplusplus_amd import LanczosEngine  # noqa: E402
from lanczosplusplus_amd._capi import check  # noqa: E402
from lanczosplusplus_amd.engine import OPERATORS, new_parts  # noqa: E402

UP = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=28)
    ap.add_argument("--m", type=int, default=14)
    ap.add_argument("--calib-stream", default="", help="path of the calib_stream binary; empty: no ratio")
    ap.add_argument("--gs-steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "many_point_heis_L28.json"))
    a = ap.parse_args()
    L, m = a.sites, a.m
    rate = stream_rate(a.calib_stream) if a.calib_stream else 0.0
    import torch  # after calib_stream: this process opens the GPU from here on

    h = L // 2
    strings = dict(four_spin=[("sz", 0, UP), ("sz", 1, UP), ("sz", h, UP), ("sz", h + 1, UP)],
                   exchange=[("splus", 0, UP), ("sminus", 1, UP), ("splus", h, UP), ("sminus", h + 1, UP)])
    eight = [[("splus", s, UP), ("sminus", s + 1, UP), ("sz", (s + h) % L, UP), ("sz", (s + h + 1) % L, UP)] for s in range(8)]
    out = dict(config="Heisenberg S=1/2 chain L=%d szPlusConst=%d J=1 open f64" % (L, m), warmup=WARMUP, repeat=REPEAT,
               strings={k: [list(o) for o in v] for k, v in strings.items()},
               stream_rate=dict(tool="scripts/calib_stream.hip", line=CALIB_LINE, kind="read, 16 bytes per lane, 4 GiB", gbs=rate) if rate else None)
    with LanczosEngine(max_steps=a.gs_steps, save_vectors=0) as e:
        j = chain(L, 1.0)
        e.assemble_heisenberg(L, m, j, j)
        out["states"] = e.rows()
        e.keep_states(1)
        eg, _, st = e.lanczos(1, want_vectors=False)
        out["ground_state"] = dict(E0=eg[0], steps=st["steps"])
        gs_ptr, n = e.state_device(0)
        bra = torch.from_numpy(e.state(0)).cuda()
        has = C.c_int32()

        for name, string in strings.items():
            # the chain: one device vector per intermediate sector, four launches, one dot
            cur, sectors = m, []
            for op, site, spin in string:
                nxt = new_parts(op, spin, L, cur, 0, basis="spin_half")
                cur = cur if nxt is None else nxt[0]
                sectors.append(cur)
            assert sectors[-1] == m
            bufs = [torch.empty(comb(L, p), dtype=torch.float64, device="cuda") for p in sectors]

            def chained_value():
                src, sp = gs_ptr, m
                for (op, site, spin), buf, nxt in zip(string, bufs, sectors):
                    check(e._lib.lpp_engine_apply_operator_heis(e._h, OPERATORS[op], site, spin, L, sp, 0, 1.0, 0.0, C.c_void_p(src), C.c_void_p(buf.data_ptr()), 0, C.byref(has)))
                    src, sp = buf.data_ptr(), nxt
                e.sync()
                v = torch.dot(bra, bufs[-1])
                torch.cuda.synchronize()
                return float(v)

            def fused_value():
                return float(e.many_point([string], basis="spin_half")[0])

            fv, cv = fused_value(), chained_value()
            values = dict(many_point=fv, chain=cv, difference=abs(fv - cv), bits_match=struct.pack("<d", fv) == struct.pack("<d", cv))
            assert abs(fv - cv) <= 1e-10 * max(abs(cv), 1e-3), values
            # (a): each is timed in its own window, back to back
            fused = timed(fused_value)
            chained = timed(chained_value)
            # (c): device events around the bracket kernel + reduction
            ms1, by1 = e.bench_string_dot([string], L, m, 0, warmup=WARMUP, iters=REPEAT, basis="spin_half")
            gbs = by1 / ms1 * 1e-6
            out[name] = dict(values=values, many_point=fused, chain=chained, chain_over_many_point=round(chained["median_ms"] / fused["median_ms"], 3),
                             many_point_not_slower=bool(fused["median_ms"] <= chained["median_ms"]), chain_intermediate_elements=sum(b.numel() for b in bufs),
                             chain_launches=len(string) + 1,
                             bytes_over_time=dict(kernel_ms=round(ms1, 4), model_bytes=by1, gbs=round(gbs, 1), ratio_to_stream=round(gbs / rate, 3) if rate else None))
            del bufs
        out["note_a"] = ("many_point: host clock around planning + upload of the run entries + bracket kernel + reduction + sync; chain: four apply_operator_heis "
                         "launches on device vectors, sync, torch.dot, sync.  bits_match: the chain's dot is torch's, another order of summation")
        out["note_c"] = "model bytes: bra read once + one gathered ket element per destination the string reaches; run entries, tables and the reduction are not counted"

        # (b): device events
        ms8, by8 = e.bench_string_dot(eight, L, m, 0, warmup=WARMUP, iters=REPEAT, basis="spin_half")
        singles = [e.bench_string_dot([s], L, m, 0, warmup=WARMUP, iters=REPEAT, basis="spin_half")[0] for s in eight]
        out["b_batching"] = dict(eight_in_one_launch_ms=round(ms8, 4), eight_launches_of_one_ms=round(sum(singles), 4), each_single_ms=[round(s, 4) for s in singles],
                                 separate_over_batched=round(sum(singles) / ms8, 3), model_bytes_batched=by8)
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
