#!/usr/bin/env python3
"""Times of the bond-orientational order on one context: nbco_bond_order_tree (the range-limited kd-tree walk with
the harmonics of the bonds at the leaves, its tree build and the summary included) on the Gaussian ball bench.py uses, at N = 2^14,
2^18 and 2^20 and rmax = 1.5, 2 and 3 times the mean particle spacing a = (V / N)^(1/3), V = 4 pi / 3 sx sy sz the volume of the
1-sigma ellipsoid.  In the same run nbco_pair_hist_tree with nn2 only at the same rmax: the same tree build and the same walk with the
cheap visitor, so the ratio is the price of the harmonics.  The exact form nbco_bond_order is timed up to --exact-max-log2.  All
three outputs are asked for.  One warm-up call per shape, then the repeats alternate between the forms; median, minimum and maximum
of the repeats.  Every timed call ends synchronised, so wall time around it is the time of the call.  `bonds` is the number of
directed bonds the call found, `ns_per_bond` the tree form's time over it.  Where both forms ran, nb is compared integer for integer
and q^2 within 1e-11.  Writes profiles/r10a_bond_order.json.

    python tools/bench_bond_order.py [--log2 14 18 20] [--exact-max-log2 14] [--repeats 7] [--out profiles/r10a_bond_order.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10a_bond_order.json"))
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
        nb = {k: torch.empty(n, dtype=torch.int32, device="cuda") for k in ("tree", "exact")}
        q = {k: torch.empty((n, 2), dtype=torch.float64, device="cuda") for k in ("tree", "exact")}
        nn2 = torch.empty(n, dtype=torch.float64, device="cuda")
        for mult in (1.5, 2.0, 3.0):
            rmax = mult * spacing
            summary = {}

            def bond(kind, fn):
                summary[kind] = fn(d, n, rmax, nb=nb[kind], q=q[kind])[2]

            calls = {"bond_tree": lambda: bond("tree", eng.bond_order_tree),
                     "pair_walk": lambda: eng.pair_hist_tree(d, n, 1, rmax, counts=False, nn2=nn2)}
            if lg <= a.exact_max_log2:
                calls["bond_exact"] = lambda: bond("exact", eng.bond_order)
            for fn in calls.values():
                fn()                              # (buffers sized, kernels loaded)
            ts = {k: [] for k in calls}
            for _ in range(a.repeats):
                for k, fn in calls.items():
                    ts[k].append(timed_ms(fn))
            s = summary["tree"]
            row = {"n": n, "rmax_over_spacing": mult, "rmax": rmax, "repeats": a.repeats, "bonds": s.bonds, "isolated": s.isolated, "nb_max": s.nb_max,
                   "q_mean": list(s.q_mean), "Q": list(s.Q)}
            for k, v in ts.items():
                row[k + "_ms"] = statistics.median(v)
                row[k + "_min_ms"], row[k + "_max_ms"] = min(v), max(v)
            row["bond_over_pair_walk"] = row["bond_tree_ms"] / row["pair_walk_ms"]
            row["ns_per_bond"] = 1e6 * row["bond_tree_ms"] / max(s.bonds, 1)
            if "bond_exact" in calls:
                row["same_nb"] = bool(torch.equal(nb["tree"], nb["exact"]))
                row["max_dq2"] = float((q["tree"] ** 2 - q["exact"] ** 2).abs().max())
                row["exact_over_tree"] = row["bond_exact_ms"] / row["bond_tree_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_bond_order.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
