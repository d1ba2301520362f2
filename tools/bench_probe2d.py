#!/usr/bin/env python3
"""Times of the 2-D probe calls for the KV beam at p = 5, field and potential both asked for, median of 5 each:
nbco_2d_probe_fmm with the particles themselves as probes (m = n = 2^20), nbco_2d_probe_fmm of the same sources on a 512 x 512
grid 1.5 x the beam's box, and the exact nbco_2d_probe at n = m = 2^16.  Every call synchronises, so wall time around it is the
time of the call.  Next to them the time of one nbco_2d_fmm evaluation at the same n as tools/bench2d.py reports it, taken first,
in a child process of this run.  Writes profiles/r06a_probe2d.json.

    python tools/bench_probe2d.py [--n 1048576] [--grid 512] [--exact-n 65536] [--order 5] [--repeats 5] [--out profiles/r06a_probe2d.json]
"""
import argparse
import json
import os
import statistics
import subprocess
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
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--exact-n", type=int, default=1 << 16)
    ap.add_argument("--order", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06a_probe2d.json"))
    a = ap.parse_args()
    # tools/bench2d.py first, in a process of its own: its fmm_eval_ms is the yardstick the probe times stand next to
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench2d.py"), "--sizes", str(a.n), "--steps", "5", "--warmup", "2",
                        "--repeats", str(a.repeats), "--exact-max", "0"], capture_output=True, text=True, check=True)
    b2d = json.loads(r.stdout.strip().splitlines()[-1])["cases"][0]
    import torch
    import bench2d
    from coulomb_oscillators_amd import Engine, init2d
    A, om, xi, om0 = bench2d.kv_params()
    eng = Engine(fmm_order=a.order, tree_radius=1.0, eps2=1e-18, coll=1, dens_inhom=1.0, tree_L=0, sync=1)
    out = {"tool": "tools/bench_probe2d.py", "device": torch.cuda.get_device_name(0), "order": a.order, "repeats": a.repeats,
           "bench2d": {k: b2d[k] for k in ("n", "L", "ms_per_step", "fmm_eval_ms", "energy_fmm_ms")}, "rows": []}

    def run(what, fn, n, x, m, t):
        prm = torch.from_numpy(np.array([xi / n, 0.0, om0[0] ** 2, om0[1] ** 2])).cuda()
        acc = torch.full((m, 2), float("nan"), dtype=torch.float64, device="cuda")
        psi = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
        med, ts = median_ms(lambda: fn(x, n, t, m, prm, acc, psi), a.repeats)
        row = {"what": what, "n": n, "m": m, "ms": med, "repeats_ms": ts, "ns_per_probe": 1e6 * med / m,
               "finite": bool(torch.isfinite(acc).all().item() and torch.isfinite(psi).all().item())}
        if n == b2d["n"]:
            row["over_fmm_eval"] = med / b2d["fmm_eval_ms"]
        out["rows"].append(row)
        print(json.dumps(row))

    st = init2d(a.n, "kv", A, om)
    x = torch.from_numpy(st[0].reshape(-1).copy()).cuda()
    run("probe_fmm at the particles", eng.probe_fmm_2d, a.n, x, a.n, x)
    mn, mx = st[0].min(0), st[0].max(0)
    ctr, half = (mn + mx) / 2, 1.5 * (mx - mn).max() / 2
    g = np.linspace(-half, half, a.grid)
    gx, gy = np.meshgrid(ctr[0] + g, ctr[1] + g, indexing="ij")
    t = torch.from_numpy(np.stack([gx.ravel(), gy.ravel()], 1).reshape(-1).copy()).cuda()
    run("probe_fmm on a %d x %d grid, 1.5 x the box" % (a.grid, a.grid), eng.probe_fmm_2d, a.n, x, a.grid * a.grid, t)
    se = init2d(a.exact_n, "kv", A, om)
    xe = torch.from_numpy(se[0].reshape(-1).copy()).cuda()
    run("probe exact at the particles", eng.probe_2d, a.exact_n, xe, a.exact_n, xe)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
