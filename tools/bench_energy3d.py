#!/usr/bin/env python3
"""Times of the 3-D energy diagnostics on one context: one nbco_fmm_kdtree rebuild evaluation, nbco_energy_fmm
(multipoles evaluated at the particles, O(N log N)), nbco_kd_potential (the O(N) pass over the locals) and nbco_energy_tree (a tree
of its own on a private context + that pass), median of 5 each, at N = 65 536 and 2^20, p = 6, on the Gaussian ball bench.py uses.
Every call synchronises, so wall time around it is the time of the call.  Writes profiles/r05a_energy3d.json.

    python tools/bench_energy3d.py [--sizes 65536 1048576] [--order 6] [--repeats 5] [--out profiles/r05a_energy3d.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, repeats):
    fn()                                   # (buffers sized, kernels loaded)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 1 << 20])
    ap.add_argument("--order", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05a_energy3d.json"))
    a = ap.parse_args()
    import torch
    import bench
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE
    rows = []
    eng = Engine(fmm_order=a.order, unsort=1, sync=1)
    for n in a.sizes:
        d = torch.from_numpy(bench.gaussian_ball(n)).cuda()
        prm = torch.from_numpy(bench.coulomb_params(n)).cuda()
        sync = torch.cuda.synchronize

        def evaluate():
            eng.compute_force(EVAL_FMM_KDTREE, d, n, prm)
            sync()
        row = {"n": n, "order": a.order, "repeats": a.repeats}
        row["fmm_eval_ms"] = median_ms(evaluate, a.repeats)
        row["energy_fmm_ms"] = median_ms(lambda: eng.energy_fmm(d, n, prm), a.repeats)
        row["kd_potential_ms"] = median_ms(lambda: eng.energy_kd(d, n, prm), a.repeats)
        row["energy_tree_ms"] = median_ms(lambda: eng.energy_tree(d, n, prm), a.repeats)
        e_old, e_new, e_tree = eng.energy_fmm(d, n, prm), eng.energy_kd(d, n, prm), eng.energy_tree(d, n, prm)
        row["coulomb_energy_fmm"], row["coulomb_kd_potential"], row["coulomb_energy_tree"] = e_old[2], float(e_new[2]), float(e_tree[2])
        row["energy_fmm_over_kd_potential"] = row["energy_fmm_ms"] / row["kd_potential_ms"]
        row["energy_tree_over_fmm_eval"] = row["energy_tree_ms"] / row["fmm_eval_ms"]
        info = eng.kd_info()
        row["m2l_pairs"], row["p2p_pairs"], row["levels"] = info.m2l_pairs, info.p2p_pairs, info.L
        rows.append(row)
        print(json.dumps(row))
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_energy3d.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
