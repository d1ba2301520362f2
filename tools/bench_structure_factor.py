#!/usr/bin/env python3
"""Times of the static structure factor on one context: nbco_structure_factor on the Gaussian ball bench.py uses, at
N = 2^14, 2^18 and 2^20 and h = (4,4,4), (8,8,8) and (16,16,16), kstep = 2 pi / (8 sigma) per axis.  One warm-up call per shape, then
the repeats alternate between the grids of one N; median, minimum and maximum of the repeats and their spread (max - min) / median.
Every timed call ends synchronised (n_used is asked for), so wall time around it is the time of the call.  `terms` is N K, the
number of (particle, wave vector) pairs; the accumulation loop spends 6 fp64 vector instructions on each (2 multiplications, 2 fused
multiply-adds, 2 additions: one complex product and one complex sum), so `fp64_fraction` is 6 terms / time over the card's fp64
vector issue rate, 256 CUs x 64 lanes per clock x 2.4 GHz = 39.3e12 per second (78.6 TFLOPS counts a fused multiply-add twice).
With --host-log2 the host route -- copy the positions, exp(i k . x) in fp64 numpy, sum -- is timed once at that N and the first grid.
Writes profiles/r11a_structure_factor.json.

    python tools/bench_structure_factor.py [--log2 14 18 20] [--repeats 7] [--host-log2 14] [--out profiles/r11a_structure_factor.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = [(4, 4, 4), (8, 8, 8), (16, 16, 16)]
FP64_LANES_PER_S = 256 * 64 * 2.4e9


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def host_route(d, n, h, kstep):
    """what a user does without the call: copy, n x K complex exponentials in fp64 numpy, in slabs of k to bound the memory"""
    import numpy as np
    x = d.cpu().numpy().reshape(-1, 3)[:n].astype(np.float64)
    ix, iy, iz = np.arange(0, h[0] + 1), np.arange(-h[1], h[1] + 1), np.arange(-h[2], h[2] + 1)
    k = np.stack(np.meshgrid(ix * kstep[0], iy * kstep[1], iz * kstep[2], indexing="ij"), axis=-1).reshape(-1, 3)
    rho = np.empty(len(k), dtype=np.complex128)
    slab = max(1, (1 << 22) // n)
    for k0 in range(0, len(k), slab):
        rho[k0:k0 + slab] = np.exp(1j * (k[k0:k0 + slab] @ x.T)).sum(axis=1)
    return rho


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[14, 18, 20])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-log2", type=int, default=14)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11a_structure_factor.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from coulomb_oscillators_amd import Engine
    rows = []
    eng = Engine(sync=1)
    kstep = [2.0 * math.pi / (8.0 * s) for s in bench.SIGMA_X]
    for lg in a.log2:
        n = 1 << lg
        d = torch.from_numpy(bench.gaussian_ball(n)[0].copy()).cuda()
        rho = {h: torch.empty((h[0] + 1) * (2 * h[1] + 1) * (2 * h[2] + 1), dtype=torch.complex128, device="cuda") for h in GRIDS}
        used = {}

        def call(h):
            used[h] = eng.structure_factor(d, n, h, kstep, rho=rho[h])[1]

        for h in GRIDS:
            call(h)                               # (buffers sized, kernels loaded)
        ts = {h: [] for h in GRIDS}
        for _ in range(a.repeats):
            for h in GRIDS:
                ts[h].append(timed_ms(lambda: call(h)))
        for h in GRIDS:
            v, K = ts[h], rho[h].numel()
            med = statistics.median(v)
            r = rho[h].cpu().numpy()
            k0 = h[1] * (2 * h[2] + 1) + h[2]
            row = {"n": n, "h": list(h), "K": K, "kstep": kstep, "repeats": a.repeats, "n_used": used[h], "ms": med, "min_ms": min(v), "max_ms": max(v),
                   "spread": (max(v) - min(v)) / med, "terms": n * K, "gterms_per_s": 1e-6 * n * K / med,
                   "fp64_fraction": 6.0 * n * K / (1e-3 * med) / FP64_LANES_PER_S,
                   "rho0": [float(r[k0].real), float(r[k0].imag)], "S_max_off_zero": float(np.delete(np.abs(r) ** 2, k0).max() / used[h])}
            if lg == a.host_log2 and h == GRIDS[0]:
                t0 = time.perf_counter()
                ref = host_route(d, n, h, kstep)
                row["host_route_ms"] = 1e3 * (time.perf_counter() - t0)
                row["host_route_max_diff"] = float(np.abs(ref - r).max())
            rows.append(row)
            print(json.dumps(row), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_structure_factor.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
