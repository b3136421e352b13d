#!/usr/bin/env python
"""Measure the many-point path of the one-orbital t-J basis at BASELINE config 4 (4x5, 9 up 9 down, t = -1, J = 0.4, W = -0.1, c128, 9.24e6 states) on
the resident ground state and write ONE JSON document (committed as profiles/many_point_tj_c4.json).  All in one run:
  (a) a pair string  c i up; c j down; cdagger l down; cdagger k up  and a hole-spin-spin string  cdagger 0 up; c 0 up; splus h; sminus h+1  through
      LanczosEngine.many_point(basis="tj") (planning, upload of the down entries, the bracket kernel, the reduction and the sync: a host clock around
      the whole call) against the same string chained through four lpp_engine_apply_operator_tj launches on device vectors plus a dot product (host
      clock around the four enqueues, the engine's sync, torch.vdot and torch's sync).  The values are compared before anything is timed -- within
      the bracket bound len * 2^-53 * |bra| * |ket| -- and whether their bits match is recorded.
  (b) 8 strings in one launch against 8 launches of one string (device events, lpp_engine_bench_string_dot_tj).
  (c) the bytes of each string of (a) -- bra once, one ket element per destination the string reaches -- over its kernel time (device events), against
      the `stream16` read rate of scripts/calib_stream.hip measured in a child process before this process opens the GPU.
Warm-up: 2 calls of every timed shape; repetition: 10 calls, every time listed, the median quoted.
Usage: hipcc --offload-arch=gfx950 -O3 -o scripts/calib_stream scripts/calib_stream.hip
       python scripts/bench_many_point_tj.py [--calib-stream scripts/calib_stream] [--out profiles/many_point_tj_c4.json] [--lx 5 --ly 4 --nup 9 --ndown 9]"""
import argparse
import ctypes as C
import json
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_many_point import REPEAT, WARMUP, timed  # noqa: E402
from bench_observables import CALIB_LINE, square, stream_rate  # noqa: E402
from lanczosplusplus_amd import LanczosEngine  # noqa: E402
from lanczosplusplus_amd._capi import check  # noqa: E402
from lanczosplusplus_amd.engine import OPERATORS, new_parts, sector_size  # noqa: E402

UP, DOWN = 0, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lx", type=int, default=5)
    ap.add_argument("--ly", type=int, default=4)
    ap.add_argument("--nup", type=int, default=9)
    ap.add_argument("--ndown", type=int, default=9)
    ap.add_argument("--calib-stream", default="", help="path of the calib_stream binary; empty: no ratio")
    ap.add_argument("--gs-steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "many_point_tj_c4.json"))
    a = ap.parse_args()
    L, parts = a.lx * a.ly, (a.nup, a.ndown)
    rate = stream_rate(a.calib_stream) if a.calib_stream else 0.0
    import torch  # after calib_stream: this process opens the GPU from here on

    h = L // 2
    strings = dict(pair=[("c", 0, UP), ("c", 1, DOWN), ("cdagger", h + 1, DOWN), ("cdagger", h, UP)],
                   hole_spin_spin=[("cdagger", 0, UP), ("c", 0, UP), ("splus", h, UP), ("sminus", h + 1, UP)])
    eight = [[("c", s, UP), ("c", s + 1, DOWN), ("cdagger", (s + h + 1) % L, DOWN), ("cdagger", (s + h) % L, UP)] for s in range(8)]
    out = dict(config="t-J %dx%d %dup %ddown t=-1 J=0.4 W=-0.1 c128" % (a.lx, a.ly, a.nup, a.ndown), warmup=WARMUP, repeat=REPEAT,
               strings={k: [list(o) for o in v] for k, v in strings.items()},
               stream_rate=dict(tool="scripts/calib_stream.hip", line=CALIB_LINE, kind="read, 16 bytes per lane, 4 GiB", gbs=rate) if rate else None)
    with LanczosEngine(dtype="c128", max_steps=a.gs_steps, save_vectors=0) as e:
        e.assemble_tj(L, a.nup, a.ndown, square(a.lx, a.ly, -1.0), square(a.lx, a.ly, 0.4), square(a.lx, a.ly, 0.4), square(a.lx, a.ly, -0.1))
        out["states"] = e.rows()
        out["layout_kernel"] = e.layout()["kernel"]
        e.keep_states_tj(1)
        eg, _, st = e.lanczos(1, want_vectors=False)
        out["ground_state"] = dict(E0=eg[0], steps=st["steps"])
        gs_ptr, n = e.state_device(0)
        gs = e.state(0)
        bra = torch.from_numpy(gs).cuda()
        bound = len(gs) * 2.0 ** -53 * float(np.linalg.norm(gs)) ** 2
        has = C.c_int32()

        for name, string in strings.items():
            # the chain: one device vector per intermediate sector, four launches, one dot
            cur, sectors = parts, []
            for op, site, spin in string:
                cur = new_parts(op, spin, L, cur[0], cur[1], basis="tj")
                assert cur is not None
                sectors.append(cur)
            assert sectors[-1] == parts
            bufs = [torch.empty(sector_size(L, p[0], p[1], "tj"), dtype=torch.complex128, device="cuda") for p in sectors]

            def chained_value():
                src, sp = gs_ptr, parts
                for (op, site, spin), buf, nxt in zip(string, bufs, sectors):
                    check(e._lib.lpp_engine_apply_operator_tj(e._h, OPERATORS[op], site, spin, L, sp[0], sp[1], 1.0, 0.0, C.c_void_p(src), C.c_void_p(buf.data_ptr()), 0,
                                                              C.byref(has)))
                    src, sp = buf.data_ptr(), nxt
                e.sync()
                v = torch.vdot(bra, bufs[-1])
                torch.cuda.synchronize()
                return complex(v)

            def fused_value():
                return complex(e.many_point([string], basis="tj")[0])

            fv, cv = fused_value(), chained_value()
            values = dict(many_point=[fv.real, fv.imag], chain=[cv.real, cv.imag], difference=abs(fv - cv), bound=bound,
                          bits_match=struct.pack("<dd", fv.real, fv.imag) == struct.pack("<dd", cv.real, cv.imag))
            assert abs(fv - cv) <= bound, values
            # (a): each is timed in its own window, back to back
            fused = timed(fused_value)
            chained = timed(chained_value)
            # (c): device events around the bracket kernel + reduction
            ms1, by1 = e.bench_string_dot([string], L, a.nup, a.ndown, warmup=WARMUP, iters=REPEAT, basis="tj")
            gbs = by1 / ms1 * 1e-6
            out[name] = dict(values=values, many_point=fused, chain=chained, chain_over_many_point=round(chained["median_ms"] / fused["median_ms"], 3),
                             many_point_not_slower=bool(fused["median_ms"] <= chained["median_ms"]), chain_intermediate_elements=sum(b.numel() for b in bufs),
                             chain_launches=len(string) + 1,
                             bytes_over_time=dict(kernel_ms=round(ms1, 4), model_bytes=by1, gbs=round(gbs, 1), ratio_to_stream=round(gbs / rate, 3) if rate else None))
            del bufs
        out["note_a"] = ("many_point: host clock around planning + upload of the down entries + bracket kernel + reduction + sync; chain: four apply_operator_tj "
                         "launches on device vectors, sync, torch.vdot, sync.  bits_match: the chain's dot is torch's, another order of summation")
        out["note_c"] = "model bytes: bra read once + one gathered ket element per destination the string reaches; down entries, word lists and the reduction are not counted"

        # (b): device events
        ms8, by8 = e.bench_string_dot(eight, L, a.nup, a.ndown, warmup=WARMUP, iters=REPEAT, basis="tj")
        singles = [e.bench_string_dot([s], L, a.nup, a.ndown, warmup=WARMUP, iters=REPEAT, basis="tj")[0] for s in eight]
        out["b_batching"] = dict(eight_in_one_launch_ms=round(ms8, 4), eight_launches_of_one_ms=round(sum(singles), 4), each_single_ms=[round(s, 4) for s in singles],
                                 separate_over_batched=round(sum(singles) / ms8, 3), model_bytes_batched=by8)
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
