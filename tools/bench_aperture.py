#!/usr/bin/env python3
"""Measurements of the aperture on one context, on the Gaussian ball bench.py uses.

(a) Call times at N = 2^20 and 2^24, beside nbco_minmax over the same positions in the same process (the one read pass over the same
    12 bytes per particle that the library had before), all with opts.sync = 1: nbco_aperture_count, an nbco_aperture_apply that
    loses nobody (an ellipsoid of 1e3 rms radii) and one that loses about 1 % (3.368 rms radii: chi^2_3 > 11.345) with the full loss
    record.  The lossy call works on a fresh copy of the state every time; the copy is outside the timed region.  Median of the
    repeats; every timed call ends synchronised, so wall time around it is the time of the call.
(b) The late phase of a run: leapfrog at N = 2^20 with tree_steps = 8 and m2l_first = 1, 1000 steps in calls of 50, then ms per step
    and p2p_pairs over the steps 1000-1020 -- without an aperture, and with an ellipsoid of 4, 6 and 8 rms radii applied after
    every 50 steps.  `lost` is the number of particles that left the run.

    python tools/bench_aperture.py [--skip-a] [--skip-b] [--log2 20 24] [--repeats 9] [--order 6] [--out profiles/r10a_aperture.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, repeats, before=None):
    ts = []
    for i in range(repeats + 1):               # (the first call sizes buffers and loads kernels: not counted)
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if i:
            ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def call_times(a, torch, bench, Engine, AP_ELLIPSOID):
    rows = []
    eng = Engine(sync=1)
    for lg in a.log2:
        n = 1 << lg
        fresh = torch.from_numpy(bench.gaussian_ball(n)).cuda().reshape(-1)
        d = fresh.clone()
        lost = torch.empty(6 * n, dtype=torch.float32, device="cuda")
        lost_row = torch.empty(n, dtype=torch.int32, device="cuda")
        far = [1e3 * s for s in bench.SIGMA_X]
        one_percent = [3.368 * s for s in bench.SIGMA_X]

        def restore():
            d.copy_(fresh)
            torch.cuda.synchronize()
        row = {"n": n, "repeats": a.repeats}
        row["minmax_ms"] = median_ms(lambda: eng.minmax(d, n), a.repeats)
        row["count_ms"] = median_ms(lambda: eng.aperture_count(d, n, AP_ELLIPSOID, far), a.repeats)
        row["apply_no_loss_ms"] = median_ms(lambda: eng.aperture(d, n, AP_ELLIPSOID, far, lost=lost, lost_row=lost_row), a.repeats)
        kept = []
        row["apply_1pct_ms"] = median_ms(lambda: kept.append(eng.aperture(d, n, AP_ELLIPSOID, one_percent, lost=lost, lost_row=lost_row)), a.repeats, restore)
        row["lost_1pct"] = n - kept[-1]
        row["no_loss_over_minmax"] = row["apply_no_loss_ms"] / row["minmax_ms"]
        row["read_GBps_no_loss"] = 12.0 * n / (row["apply_no_loss_ms"] * 1e-3) / 1e9
        rows.append(row)
        print(json.dumps(row), flush=True)
        del fresh, d, lost, lost_row
    eng.close()
    return rows


def late_phase(a, torch, bench, Engine, AP_ELLIPSOID):
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE, INTEG_LEAPFROG
    rows = []
    n0 = 1 << 20
    for radii in (None, 4.0, 6.0, 8.0):
        eng = Engine(fmm_order=a.order, unsort=0, tree_steps=8, m2l_first=1, sync=0)
        d = torch.from_numpy(bench.gaussian_ball(n0)).cuda().reshape(-1)
        prm = torch.from_numpy(bench.coulomb_params(n0)).cuda()
        half = None if radii is None else [radii * s for s in bench.SIGMA_X]
        n = n0
        eng.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        for _ in range(1000 // 50):
            eng.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, 5e-4, 50)
            if half:
                n = eng.aperture(d, n, AP_ELLIPSOID, half)
        eng.sync()
        t0 = time.perf_counter()
        eng.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, 5e-4, 20)
        eng.sync()
        ms = 1e3 * (time.perf_counter() - t0) / 20
        info = eng.kd_info()
        row = {"n0": n0, "order": a.order, "aperture_rms_radii": radii, "lost": n0 - n, "n_left": n, "ms_per_step_1000_1020": ms,
               "p2p_pairs": int(info.p2p_pairs), "m2l_pairs": int(info.m2l_pairs)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        eng.close()
        del d
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--order", type=int, default=6)
    ap.add_argument("--skip-a", action="store_true")
    ap.add_argument("--skip-b", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10a_aperture.json"))
    a = ap.parse_args()
    import torch
    import bench
    from coulomb_oscillators_amd import AP_ELLIPSOID, Engine
    out = {"tool": "tools/bench_aperture.py", "device": torch.cuda.get_device_name(0)}
    if not a.skip_a:
        out["call_times"] = call_times(a, torch, bench, Engine, AP_ELLIPSOID)
    if not a.skip_b:
        out["late_phase"] = late_phase(a, torch, bench, Engine, AP_ELLIPSOID)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
