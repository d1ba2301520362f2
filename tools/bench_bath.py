#!/usr/bin/env python3
"""Measurements of the Langevin bath (DESIGN, "Langevin bath"), on the Gaussian ball bench.py uses.

(a) nbco_bath_apply beside nbco_step on v (v += a s: the kick, the pass over v of the same size) at N = 2^20 and 2^24, opts.sync = 0:
    `calls` calls enqueued, one synchronise, wall time / calls; the two in turns, median of the repeats.  The bath reads and writes v
    (24 bytes per particle) and draws three Philox blocks per particle, the step reads a and reads and writes v (36): GB/s for each.
(b) One leapfrog step at N = 2^20, opts.unsort = 0, m2l_first = 1, tree_steps 1 and 8, four legs: `plain` (nbco_integrate_steps), `bath`
    (nbco_integrate_steps_t: the bath's half steps inside the fused pass), `bath_looped` (as many calls of nbco_integrate_t: the half
    steps as launches of their own, no fused pass) and `bath_field` (nbco_integrate_steps_t with Omega).  Every bath leg runs beside a
    plain leg of its own, two engines from the same state alive at a time (as tools/bench_bfield.py); after a warm-up of `warm` steps
    each, windows of `steps` steps in turns, median of the repeats and the range.  The rates
    are small (gamma dt = 0.01) and the bath cold, so that the balls stay alike over the measurement and the trees, which set the cost of
    a step, stay comparable; the values do not enter the cost of the bath itself.

    python tools/bench_bath.py [--skip-a] [--skip-b] [--log2 20 24] [--repeats 5] [--order 6] [--out profiles/r13a_bath.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAMMA, KT, SEED = (20.0, 20.0, 20.0), (1e-10, 1e-10, 1e-10), 12345
OMEGA = (30.0, -20.0, 93.0)      # |Omega| dt = 0.05 at bench.py's dt = 5e-4, as tools/bench_bfield.py
DT = 5e-4


def timed(eng, fn, calls):
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    eng.sync()
    return 1e3 * (time.perf_counter() - t0) / calls


def apply_times(a, torch, bench, Engine):
    rows = []
    eng = Engine(sync=0)
    for lg in a.log2:
        n = 1 << lg
        d = torch.from_numpy(bench.gaussian_ball(n)).cuda().reshape(-1)
        v, acc = d[3 * n:6 * n], d[:3 * n]
        calls = max(20, (1 << 31) // n)
        legs = {"step": lambda: eng.step(v, acc, 1e-9, n), "bath_apply": lambda: eng.bath_apply(v, n, GAMMA, KT, 0.5 * DT, 0, 3, seed=SEED)}
        ms = {k: [] for k in legs}
        for k, fn in legs.items():      # (first calls load the kernels: not counted)
            timed(eng, fn, 3)
        for _ in range(a.repeats):
            for k, fn in legs.items():
                ms[k].append(timed(eng, fn, calls))
        row = {"n": n, "calls": calls, "repeats": a.repeats}
        for k, nbytes in (("step", 36.0), ("bath_apply", 24.0)):
            med = statistics.median(ms[k])
            row[k + "_ms"] = med
            row[k + "_ms_range"] = [min(ms[k]), max(ms[k])]
            row[k + "_GBps"] = nbytes * n / (med * 1e-3) / 1e9
        row["bath_apply_over_step"] = row["bath_apply_ms"] / row["step_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del d, v, acc
    eng.close()
    return rows


def step_times(a, torch, bench, Engine):
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE, INTEG_LEAPFROG
    rows = []
    n = 1 << 20
    L, K = INTEG_LEAPFROG, EVAL_FMM_KDTREE
    prm = torch.from_numpy(bench.coulomb_params(n)).cuda()
    for tree_steps in (1, 8):
        row = {"n": n, "order": a.order, "tree_steps": tree_steps, "steps_per_window": a.steps, "repeats": a.repeats}
        # every bath leg beside a plain leg of its own, two engines alive at a time (as tools/bench_bfield.py): with the engines of all four
        # legs alive at once, one leg or another -- the plain one included -- came out two to three times slower (an engine owns two
        # streams, the process has four hardware queues)
        for leg in ("bath", "bath_looped", "bath_field"):
            engs, bufs, tick = {}, {}, {"plain": 0, leg: 0}
            for k in ("plain", leg):
                engs[k] = Engine(fmm_order=a.order, unsort=0, tree_steps=tree_steps, m2l_first=1, sync=0)
                bufs[k] = torch.from_numpy(bench.gaussian_ball(n)).cuda().reshape(-1)
                engs[k].compute_force(K, bufs[k], n, prm)

            def plain(s):
                engs["plain"].integrate_steps(L, K, bufs["plain"], n, prm, DT, s)

            def bath(s):
                if leg == "bath_looped":
                    for i in range(s):
                        engs[leg].integrate_t(L, K, bufs[leg], n, prm, DT, GAMMA, KT, tick[leg] + i, seed=SEED)
                else:
                    engs[leg].integrate_steps_t(L, K, bufs[leg], n, prm, DT, s, GAMMA, KT, tick[leg], seed=SEED, omega=OMEGA if leg == "bath_field" else None)
            run = {"plain": plain, leg: bath}

            def go(k, s):
                run[k](s)
                tick[k] += s
            ms = {k: [] for k in run}
            for k in run:
                go(k, a.warm)
                engs[k].sync()
            for _ in range(a.repeats):
                for k in run:
                    ms[k].append(timed(engs[k], lambda: go(k, a.steps), 1) / a.steps)
            for k, name in (("plain", "plain_beside_" + leg), (leg, leg)):
                row[name + "_ms_per_step"] = statistics.median(ms[k])
                row[name + "_ms_per_step_range"] = [min(ms[k]), max(ms[k])]
            row[leg + "_over_plain"] = row[leg + "_ms_per_step"] / row["plain_beside_" + leg + "_ms_per_step"]
            for k in run:
                engs[k].close()
            del bufs
        rows.append(row)
        print(json.dumps(row), flush=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13a_bath.json"))
    a = ap.parse_args()
    import torch
    import bench
    from coulomb_oscillators_amd import Engine
    out = {"tool": "tools/bench_bath.py", "device": torch.cuda.get_device_name(0), "gamma": list(GAMMA), "kT": list(KT), "omega": list(OMEGA)}
    if not a.skip_a:
        out["apply"] = apply_times(a, torch, bench, Engine)
    if not a.skip_b:
        out["step"] = step_times(a, torch, bench, Engine)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
