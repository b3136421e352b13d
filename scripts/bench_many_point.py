#!/usr/bin/env python
"""Measure the many-point path at BASELINE config 2 (4x4 Hubbard, 8 up 8 down, U = 4, 1.66e8 states) on the resident ground state and write ONE JSON
document (committed as profiles/many_point_c2.json).  All in one run:
  (a) one four-operator pair string  <gs| cdagger_{l up} cdagger_{k down} c_{j down} c_{i up} |gs>  through LanczosEngine.many_point (planning, table
      upload, the bracket kernel, the reduction and the sync: a host clock around the whole call) against the same string chained through the four
      lpp_engine_apply_operator launches on device vectors plus a dot product, the only way before many_point existed (host clock around the four
      enqueues, the engine's sync, torch.dot and torch's sync).  The two values are compared before anything is timed.
  (b) 8 strings in one launch against 8 launches of one string (device events, lpp_engine_bench_string_dot).
  (c) the bytes of (a) -- bra once, one ket element per destination the string reaches -- over its kernel time (device events), against the
      `stream16` read rate of scripts/calib_stream.hip measured in a child process before this process opens the GPU.
Warm-up: 2 calls of every timed shape; repetition: 10 calls, every time listed, the median quoted.
Usage: hipcc --offload-arch=gfx950 -O3 -o scripts/calib_stream scripts/calib_stream.hip
       python scripts/bench_many_point.py [--calib-stream scripts/calib_stream] [--out profiles/many_point_c2.json] [--lx 4 --ly 4 --nup 8 --ndown 8]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from math import comb

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_observables import CALIB_LINE, square, stream_rate  # noqa: E402
from lanczosplusplus_amd import LanczosEngine  # noqa: E402
from lanczosplusplus_amd._capi import check  # noqa: E402
from lanczosplusplus_amd.engine import OPERATORS, new_parts  # noqa: E402

UP, DOWN = 0, 1
WARMUP, REPEAT = 2, 10


def timed(fn):
    for _ in range(WARMUP):
        fn()
    times = []
    for _ in range(REPEAT):
        t0 = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return dict(median_ms=round(statistics.median(times), 4), all_ms=[round(t, 4) for t in times])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lx", type=int, default=4)
    ap.add_argument("--ly", type=int, default=4)
    ap.add_argument("--nup", type=int, default=8)
    ap.add_argument("--ndown", type=int, default=8)
    ap.add_argument("--calib-stream", default="", help="path of the calib_stream binary; empty: no ratio")
    ap.add_argument("--gs-steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "many_point_c2.json"))
    a = ap.parse_args()
    L = a.lx * a.ly
    rate = stream_rate(a.calib_stream) if a.calib_stream else 0.0
    import torch  # after calib_stream: this process opens the GPU from here on

    i, j, k, l = 0, 1, L // 2 + 1, L // 2
    pair = [("c", i, UP), ("c", j, DOWN), ("cdagger", k, DOWN), ("cdagger", l, UP)]
    eight = [[("c", s, UP), ("c", (s + 1) % L, DOWN), ("cdagger", (s + 6) % L, DOWN), ("cdagger", (s + 5) % L, UP)] for s in range(8)]
    out = dict(config="%dx%d %dup %ddown U=4 f64" % (a.lx, a.ly, a.nup, a.ndown), warmup=WARMUP, repeat=REPEAT, pair_string=[list(o) for o in pair],
               stream_rate=dict(tool="scripts/calib_stream.hip", line=CALIB_LINE, kind="read, 16 bytes per lane, 4 GiB", gbs=rate) if rate else None)
    with LanczosEngine(max_steps=a.gs_steps, save_vectors=0) as e:
        e.assemble_hubbard(L, a.nup, a.ndown, square(a.lx, a.ly, -1.0), np.full(L, 4.0))
        out["states"] = e.rows()
        e.keep_states(1)
        t0 = time.time()
        eg, _, st = e.lanczos(1, want_vectors=False)
        out["ground_state"] = dict(E0=eg[0], steps=st["steps"], seconds=round(time.time() - t0, 3))
        gs_ptr, n = e.state_device(0)

        # the chain: one device vector per intermediate sector, four launches, one dot
        parts, sectors = (a.nup, a.ndown), []
        for op, site, spin in pair:
            parts = new_parts(op, spin, L, *parts)
            sectors.append(parts)
        assert sectors[-1] == (a.nup, a.ndown)
        bufs = [torch.empty(comb(L, p[0]) * comb(L, p[1]), dtype=torch.float64, device="cuda") for p in sectors]
        bra = torch.from_numpy(e.state(0)).cuda()
        has = C.c_int32()

        def chain():
            src, sp = gs_ptr, (a.nup, a.ndown)
            for (op, site, spin), buf, nxt in zip(pair, bufs, sectors):
                check(e._lib.lpp_engine_apply_operator(e._h, OPERATORS[op], site, spin, L, sp[0], sp[1], 1.0, 0.0, C.c_void_p(src), C.c_void_p(buf.data_ptr()), 0, C.byref(has)))
                src, sp = buf.data_ptr(), nxt
            e.sync()
            v = torch.dot(bra, bufs[-1])
            torch.cuda.synchronize()
            return float(v)

        fused_value, chain_value = float(e.many_point([pair])[0]), chain()
        out["values"] = dict(many_point=fused_value, chain=chain_value, difference=abs(fused_value - chain_value))
        assert abs(fused_value - chain_value) <= 1e-10 * max(abs(chain_value), 1e-3), out["values"]

        # (a): alternating would interleave the allocations of many_point with the chain's launches; each is timed in its own window, back to back
        fused = timed(lambda: e.many_point([pair]))
        chained = timed(chain)
        chain_vectors = sum(b.numel() for b in bufs)
        out["a_pair_string"] = dict(many_point=fused, chain=chained, chain_over_many_point=round(chained["median_ms"] / fused["median_ms"], 3),
                                    many_point_not_slower=bool(fused["median_ms"] <= chained["median_ms"]),
                                    chain_intermediate_elements=chain_vectors, chain_launches=len(pair) + 1,
                                    note="many_point: host clock around planning + upload + bracket kernel + reduction + sync; chain: four apply_operator "
                                         "launches on device vectors, sync, torch.dot, sync")

        # (b), (c): device events
        ms1, by1 = e.bench_string_dot([pair], L, a.nup, a.ndown, warmup=WARMUP, iters=REPEAT)
        ms8, by8 = e.bench_string_dot(eight, L, a.nup, a.ndown, warmup=WARMUP, iters=REPEAT)
        singles = [e.bench_string_dot([s], L, a.nup, a.ndown, warmup=WARMUP, iters=REPEAT)[0] for s in eight]
        out["b_batching"] = dict(eight_in_one_launch_ms=round(ms8, 4), eight_launches_of_one_ms=round(sum(singles), 4), each_single_ms=[round(s, 4) for s in singles],
                                 separate_over_batched=round(sum(singles) / ms8, 3), model_bytes_batched=by8)
        gbs = by1 / ms1 * 1e-6
        out["c_bytes_over_time"] = dict(kernel_ms=round(ms1, 4), model_bytes=by1, gbs=round(gbs, 1), ratio_to_stream=round(gbs / rate, 3) if rate else None,
                                        note="model bytes: bra read once + one gathered ket element per destination the string reaches; tables and the reduction are not counted")
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
