#!/usr/bin/env python3
"""Measurements of the uniform magnetic field (DESIGN, "Uniform magnetic field"), on the Gaussian ball bench.py uses.

(a) nbco_drift_b beside nbco_step over the same arrays (x += v s: the drift it replaces) at N = 2^20 and 2^24, opts.sync = 0: `calls`
    calls enqueued, one synchronise, wall time / calls; the two in turns, median of the repeats.  The drift reads and writes x and v
    (48 bytes per particle), the step reads v and reads and writes x (36): GB/s is given for each.
(b) One step of nbco_integrate_steps_b beside nbco_integrate_steps on the same tree: N = 2^20, leapfrog, opts.unsort = 0, m2l_first = 1,
    tree_steps 1 and 8.  Two engines from the same state; after a warm-up of `warm` steps each, windows of `steps` steps in turns,
    median of the repeats and the range.  The field's size does not enter the cost; it is small enough (|Omega| dt = 0.05) that the two
    balls stay alike over the measurement and the trees, which set the cost of a step, stay comparable.

    python tools/bench_bfield.py [--skip-a] [--skip-b] [--log2 20 24] [--repeats 5] [--order 6] [--out profiles/r12a_bfield.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OMEGA = (30.0, -20.0, 93.0)      # |Omega| = 100 per unit of time: |Omega| dt = 0.05 at bench.py's dt = 5e-4


def timed(eng, fn, calls):
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    eng.sync()
    return 1e3 * (time.perf_counter() - t0) / calls


def drift_times(a, torch, bench, Engine):
    rows = []
    eng = Engine(sync=0)
    for lg in a.log2:
        n = 1 << lg
        d = torch.from_numpy(bench.gaussian_ball(n)).cuda().reshape(-1)
        x, v = d[:3 * n], d[3 * n:6 * n]
        calls = max(20, (1 << 31) // n)
        legs = {"step": lambda: eng.step(x, v, 1e-6, n), "drift_b": lambda: eng.drift_b(x, v, n, OMEGA, 1e-6)}
        ms = {k: [] for k in legs}
        for k, fn in legs.items():      # (first calls load the kernels: not counted)
            timed(eng, fn, 3)
        for _ in range(a.repeats):
            for k, fn in legs.items():
                ms[k].append(timed(eng, fn, calls))
        row = {"n": n, "calls": calls, "repeats": a.repeats}
        for k, nbytes in (("step", 36.0), ("drift_b", 48.0)):
            med = statistics.median(ms[k])
            row[k + "_ms"] = med
            row[k + "_ms_range"] = [min(ms[k]), max(ms[k])]
            row[k + "_GBps"] = nbytes * n / (med * 1e-3) / 1e9
        row["drift_b_over_step"] = row["drift_b_ms"] / row["step_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del d, x, v
    eng.close()
    return rows


def step_times(a, torch, bench, Engine):
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE, INTEG_LEAPFROG
    rows = []
    n = 1 << 20
    for tree_steps in (1, 8):
        engs, bufs = {}, {}
        prm = torch.from_numpy(bench.coulomb_params(n)).cuda()
        for k in ("plain", "field"):
            engs[k] = Engine(fmm_order=a.order, unsort=0, tree_steps=tree_steps, m2l_first=1, sync=0)
            bufs[k] = torch.from_numpy(bench.gaussian_ball(n)).cuda().reshape(-1)
            engs[k].compute_force(EVAL_FMM_KDTREE, bufs[k], n, prm)
        run = {"plain": lambda s: engs["plain"].integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, bufs["plain"], n, prm, 5e-4, s),
               "field": lambda s: engs["field"].integrate_steps_b(INTEG_LEAPFROG, EVAL_FMM_KDTREE, bufs["field"], n, prm, 5e-4, s, OMEGA)}
        ms = {k: [] for k in run}
        for k in run:
            run[k](a.warm)
            engs[k].sync()
        for _ in range(a.repeats):
            for k in run:
                ms[k].append(timed(engs[k], lambda: run[k](a.steps), 1) / a.steps)
        row = {"n": n, "order": a.order, "tree_steps": tree_steps, "steps_per_window": a.steps, "repeats": a.repeats}
        for k in run:
            row[k + "_ms_per_step"] = statistics.median(ms[k])
            row[k + "_ms_per_step_range"] = [min(ms[k]), max(ms[k])]
        row["field_over_plain"] = row["field_ms_per_step"] / row["plain_ms_per_step"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        for k in run:
            engs[k].close()
        del bufs
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--order", type=int, default=6)
    ap.add_argument("--warm", type=int, default=16)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--skip-a", action="store_true")
    ap.add_argument("--skip-b", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12a_bfield.json"))
    a = ap.parse_args()
    import torch
    import bench
    from coulomb_oscillators_amd import Engine
    out = {"tool": "tools/bench_bfield.py", "device": torch.cuda.get_device_name(0), "omega": list(OMEGA)}
    if not a.skip_a:
        out["drift"] = drift_times(a, torch, bench, Engine)
    if not a.skip_b:
        out["step"] = step_times(a, torch, bench, Engine)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
