#!/usr/bin/env python3
"""Times of the 3-D probe calls on the Gaussian ball bench.py uses, at p = 6, field and potential both asked for,
median of 5 each: nbco_probe_tree with the particles themselves as probes (m = n = 2^20), nbco_probe_tree of the same sources on a
128^3 grid 1.5 x the ball's box, and the exact nbco_probe at n = m = 2^16.  Every call synchronises, so wall time around it is the
time of the call.  Next to them the time of one nbco_fmm_kdtree rebuild evaluation at the same n, taken first in the same session.
Writes profiles/r07a_probe3d.json.

    python tools/bench_probe3d.py [--n 1048576] [--grid 128] [--exact-n 65536] [--order 6] [--repeats 5] [--out profiles/r07a_probe3d.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, repeats):
    fn()                                   # (buffers sized, kernels loaded)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--exact-n", type=int, default=1 << 16)
    ap.add_argument("--order", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07a_probe3d.json"))
    a = ap.parse_args()
    import torch
    import bench
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE
    eng = Engine(fmm_order=a.order, unsort=1, sync=1)
    n = a.n
    st = bench.gaussian_ball(n)
    d = torch.from_numpy(st).cuda()
    prm = torch.from_numpy(bench.coulomb_params(n)).cuda()

    def evaluate():
        eng.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        torch.cuda.synchronize()
    eval_ms, eval_ts = median_ms(evaluate, a.repeats)
    info = eng.kd_info()
    out = {"tool": "tools/bench_probe3d.py", "device": torch.cuda.get_device_name(0), "order": a.order, "repeats": a.repeats,
           "fmm_eval": {"n": n, "ms": eval_ms, "repeats_ms": eval_ts, "levels": info.L, "mlt_max": info.mlt_max}, "rows": []}
    print(json.dumps(out["fmm_eval"]))

    def run(what, fn, nn, x, m, t, p):
        acc = torch.full((m, 3), float("nan"), dtype=torch.float64, device="cuda")
        psi = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
        med, ts = median_ms(lambda: fn(x, nn, t, m, p, acc, psi), a.repeats)
        row = {"what": what, "n": nn, "m": m, "ms": med, "repeats_ms": ts, "ns_per_probe": 1e6 * med / m,
               "finite": bool(torch.isfinite(acc).all().item() and torch.isfinite(psi).all().item())}
        if nn == n:
            row["over_fmm_eval"] = med / eval_ms
        out["rows"].append(row)
        print(json.dumps(row))

    pos = np.ascontiguousarray(st.reshape(-1)[:3 * n].reshape(n, 3))
    x = torch.from_numpy(pos).cuda()
    run("probe_tree at the particles", eng.probe_tree, n, x, n, x, prm)
    mn, mx = pos.min(0).astype(np.float64), pos.max(0).astype(np.float64)
    ctr, half = (mn + mx) / 2, 1.5 * (mx - mn) / 2
    g = np.linspace(-1.0, 1.0, a.grid)
    gx, gy, gz = np.meshgrid(ctr[0] + half[0] * g, ctr[1] + half[1] * g, ctr[2] + half[2] * g, indexing="ij")
    t = torch.from_numpy(np.stack([gx.ravel(), gy.ravel(), gz.ravel()], 1).astype(np.float32)).cuda()
    run("probe_tree on a %d^3 grid, 1.5 x the box" % a.grid, eng.probe_tree, n, x, a.grid ** 3, t, prm)
    ne = a.exact_n
    xe = torch.from_numpy(np.ascontiguousarray(bench.gaussian_ball(ne).reshape(-1)[:3 * ne])).cuda()
    run("probe exact at the particles", eng.probe, ne, xe, ne, xe, torch.from_numpy(bench.coulomb_params(ne)).cuda())
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
