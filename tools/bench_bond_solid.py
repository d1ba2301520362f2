#!/usr/bin/env python3
"""Times of the crystalline-particle detection on one context: nbco_bond_solid_tree with vec = NULL -- one kd-tree
build, the walk with the harmonics of the bonds (pass 1, the records in tree order), the walk over the records (pass 2) and the
summary -- on the Gaussian ball bench.py uses, at N = 2^14, 2^18 and 2^20 and rmax = 1.5, 2 and 3 times the mean particle spacing
a = (V / N)^(1/3), V = 4 pi / 3 sx sy sz the volume of the 1-sigma ellipsoid.  In the same run nbco_bond_order_tree at the same rmax:
the same tree build and pass 1 alone, so the ratio is 1 + the price of pass 2 over pass 1.  The exact form nbco_bond_solid is timed up
to --exact-max-log2.  All outputs are asked for.  One warm-up call per shape, then the repeats alternate between the forms; median,
minimum and maximum of the repeats.  Every timed call ends synchronised, so wall time around it is the time of the call.  `bonds` is the
number of directed bonds, `ns_per_bond` the solid tree form's time over it.  Where both forms ran, nb is compared integer for integer,
the particles whose xi differ are counted (each form's own records differ by rounding) and the largest |delta q-bar^2| is reported.  Writes profiles/bond_solid.json.

    python tools/bench_bond_solid.py [--log2 14 18 20] [--exact-max-log2 14] [--repeats 7] [--dmin 0.7] [--xi-min 7] [--out profiles/bond_solid.json]
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


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[14, 18, 20])
    ap.add_argument("--exact-max-log2", type=int, default=14)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dmin", type=float, default=0.7)
    ap.add_argument("--xi-min", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bond_solid.json"))
    a = ap.parse_args()
    import torch
    import bench
    from coulomb_oscillators_amd import Engine
    rows = []
    eng = Engine(sync=1)
    volume = 4.0 * math.pi / 3.0 * bench.SIGMA_X[0] * bench.SIGMA_X[1] * bench.SIGMA_X[2]
    for lg in a.log2:
        n = 1 << lg
        d = torch.from_numpy(bench.gaussian_ball(n)[0].copy()).cuda()
        spacing = (volume / n) ** (1.0 / 3.0)
        nb = {k: torch.empty(n, dtype=torch.int32, device="cuda") for k in ("tree", "exact", "order")}
        xi = {k: torch.empty(n, dtype=torch.int32, device="cuda") for k in ("tree", "exact")}
        qbar = {k: torch.empty((n, 2), dtype=torch.float64, device="cuda") for k in ("tree", "exact")}
        q = torch.empty((n, 2), dtype=torch.float64, device="cuda")
        for mult in (1.5, 2.0, 3.0):
            rmax = mult * spacing
            summary = {}

            def solid(kind, fn):
                summary[kind] = fn(d, n, rmax, a.dmin, a.xi_min, nb=nb[kind], xi=xi[kind], qbar=qbar[kind])[3]

            calls = {"solid_tree": lambda: solid("tree", eng.bond_solid_tree),
                     "bond_tree": lambda: eng.bond_order_tree(d, n, rmax, nb=nb["order"], q=q)}
            if lg <= a.exact_max_log2:
                calls["solid_exact"] = lambda: solid("exact", eng.bond_solid)
            for fn in calls.values():
                fn()                              # (buffers sized, kernels loaded)
            ts = {k: [] for k in calls}
            for _ in range(a.repeats):
                for k, fn in calls.items():
                    ts[k].append(timed_ms(fn))
            s = summary["tree"]
            row = {"n": n, "rmax_over_spacing": mult, "rmax": rmax, "repeats": a.repeats, "dmin": a.dmin, "xi_min": a.xi_min, "bonds": s.bonds,
                   "isolated": s.isolated, "solid_bonds": s.solid_bonds, "n_solid": s.n_solid, "xi_max": s.xi_max, "qbar_mean": list(s.qbar_mean)}
            for k, v in ts.items():
                row[k + "_ms"] = statistics.median(v)
                row[k + "_min_ms"], row[k + "_max_ms"] = min(v), max(v)
            row["solid_over_bond_tree"] = row["solid_tree_ms"] / row["bond_tree_ms"]
            row["ns_per_bond"] = 1e6 * row["solid_tree_ms"] / max(s.bonds, 1)
            row["same_nb_as_bond_order"] = bool(torch.equal(nb["tree"], nb["order"]))
            if "solid_exact" in calls:
                # (the records of the two forms differ by rounding: xi may differ where a d6 lies within that of dmin)
                row["same_nb"] = bool(torch.equal(nb["tree"], nb["exact"]))
                row["xi_differ"] = int((xi["tree"] != xi["exact"]).sum())
                row["max_dqbar2"] = float((qbar["tree"] ** 2 - qbar["exact"] ** 2).abs().max())
                row["exact_over_tree"] = row["solid_exact_ms"] / row["solid_tree_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_bond_solid.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
