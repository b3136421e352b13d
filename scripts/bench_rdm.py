#!/usr/bin/env python
"""Measure the reduced density matrix at BASELINE config 2 (4x4 cluster, 8 up 8 down, 1.66e8 states) for the cuts at sites 4 and 8, write
profiles/rdm_c2.json and print the same JSON on one line.  Per cut:
  kernel      ms per call and multiply-adds per second of LanczosEngine.bench_rdm (HIP events, resident pseudo-random vector)
  torch       the yardstick: the same packed result from torch on the same device -- per block an index gather that materialises V (d x K), then
              torch.matmul(V, V.T); timed with torch events, warm
  deviation   the largest |kernel - torch| over the packed result, both computed in this process from ONE vector on the device
              (LanczosEngine.reduced_density_matrix_device on the torch tensor's address), next to the largest diagonal element
Usage: python scripts/bench_rdm.py [--sites 16 --nup 8 --ndown 8 --splits 4 8] [--out profiles/rdm_c2.json]"""
import argparse
import json
import os
import sys
from math import comb

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lanczosplusplus_amd import LanczosEngine, rdm_plan  # noqa: E402


def torch_blocks(psi, plan, n_up, out):
    """the packed blocks through a vendor GEMM: V is gathered into a matrix of its own first"""
    dev = psi.device
    for b in plan["blocks"]:
        su = torch.as_tensor(plan["starts_up"][b["k_up"]], device=dev)
        sd = torch.as_tensor(plan["starts_down"][b["k_down"]], device=dev)
        iu = torch.arange(b["dim_up"], device=dev)[:, None] + su[None, :]
        idn = (torch.arange(b["dim_down"], device=dev)[:, None] + sd[None, :]) * n_up
        idx = (iu[None, :, None, :] + idn[:, None, :, None]).reshape(b["dim"], b["terms"])
        v = psi[idx]
        out[b["offset"]:b["offset"] + b["dim"] ** 2] = torch.matmul(v, v.T).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=16)
    ap.add_argument("--nup", type=int, default=8)
    ap.add_argument("--ndown", type=int, default=8)
    ap.add_argument("--splits", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rdm_c2.json"))
    a = ap.parse_args()
    L, nup, ndown = a.sites, a.nup, a.ndown
    n_up, n = comb(L, nup), comb(L, nup) * comb(L, ndown)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    psi = torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5
    psi /= torch.linalg.norm(psi)
    res = dict(config="%d sites %dup %ddown, f64" % (L, nup, ndown), states=n, device=torch.cuda.get_device_name(0), cuts={})
    with LanczosEngine() as e:
        for split in a.splits:
            plan = rdm_plan(L, nup, ndown, split)
            ms, macs = e.bench_rdm(L, nup, ndown, split, warmup=1, iters=a.iters)
            mine = torch.zeros(plan["total"], dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            e.reduced_density_matrix_device(psi.data_ptr(), mine.data_ptr(), L, nup, ndown, split)
            e.sync()
            ref = torch.zeros(plan["total"], dtype=torch.float64, device=dev)
            torch_blocks(psi, plan, n_up, ref)  # warm: allocator, GEMM selection
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                torch_blocks(psi, plan, n_up, ref)
            t1.record()
            torch.cuda.synchronize()
            tms = t0.elapsed_time(t1) / a.iters
            dmax = max(b["dim"] for b in plan["blocks"])
            diag = max(float(ref[b["offset"]:b["offset"] + b["dim"] ** 2:b["dim"] + 1].max()) for b in plan["blocks"])
            res["cuts"][str(split)] = dict(blocks=len(plan["blocks"]), largest_block=dmax, packed_elements=plan["total"], multiply_adds=macs,
                                           kernel_ms=round(ms, 3), kernel_gmacs_per_s=round(macs / ms * 1e-6, 1), torch_ms=round(tms, 3),
                                           torch_gmacs_per_s=round(macs / tms * 1e-6, 1), kernel_over_torch=round(ms / tms, 3),
                                           max_deviation=float((mine - ref).abs().max()), largest_diagonal=diag,
                                           hermitian_bit_for_bit=bool(all(torch.equal(m, m.T) for m in (mine[b["offset"]:b["offset"] + b["dim"] ** 2].view(b["dim"], b["dim"]) for b in plan["blocks"][:8]))))
            del mine, ref
            torch.cuda.empty_cache()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
