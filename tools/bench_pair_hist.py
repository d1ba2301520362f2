#!/usr/bin/env python3
"""Times of the pair statistics on one context: nbco_pair_hist (all pairs) and nbco_pair_hist_tree (the
range-limited kd-tree walk, its tree build included) on the Gaussian ball bench.py uses, at N = 2^14 .. 2^20 -- the exact form only
up to 2^18 -- with bins = 256 and rmax = 1, 2 and 4 times the mean particle spacing a = (V / N)^(1/3), V = 4 pi / 3 sx sy sz the
volume of the 1-sigma ellipsoid.  Both outputs are asked for.  Median of the repeats; every timed call ends synchronised, so wall
time around it is the time of the call.  `inside` is the number of pairs below rmax, `pairs_per_s` for the exact form the
n (n - 1) / 2 pairs it evaluates over its time.  Where both forms ran, their bytes are compared.  Writes profiles/r09a_pair_hist.json.

    python tools/bench_pair_hist.py [--log2 14 16 18 20] [--exact-max-log2 18] [--repeats 5] [--out profiles/r09a_pair_hist.json]
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


def times_ms(fn, repeats):
    """(median, minimum, maximum) of the repeats, after one warm-up call"""
    fn()                                   # (buffers sized, kernels loaded)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[14, 15, 16, 17, 18, 19, 20])
    ap.add_argument("--exact-max-log2", type=int, default=18)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09a_pair_hist.json"))
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
        forms = [("tree", eng.pair_hist_tree)] + ([("exact", eng.pair_hist)] if lg <= a.exact_max_log2 else [])
        for mult in (1, 2, 4):
            rmax = mult * spacing
            row = {"n": n, "bins": a.bins, "rmax_over_spacing": mult, "rmax": rmax, "repeats": a.repeats}
            out = {}
            for name, fn in forms:
                counts = torch.empty(a.bins + 1, dtype=torch.int64, device="cuda")
                nn2 = torch.empty(n, dtype=torch.float64, device="cuda")
                row[name + "_ms"], row[name + "_min_ms"], row[name + "_max_ms"] = times_ms(lambda: fn(d, n, a.bins, rmax, counts=counts, nn2=nn2), a.repeats)
                out[name] = (counts.cpu(), nn2.cpu())
            row["inside"] = int(out["tree"][0][:-1].sum())
            row["with_a_neighbour"] = int(torch.isfinite(out["tree"][1]).sum())
            if "exact" in out:
                row["same_bytes"] = bool(torch.equal(out["tree"][0], out["exact"][0])
                                         and torch.equal(out["tree"][1].view(torch.int64), out["exact"][1].view(torch.int64)))
                row["exact_pairs_per_s"] = n * (n - 1) / 2 / (row["exact_ms"] * 1e-3)
                row["exact_over_tree"] = row["exact_ms"] / row["tree_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_pair_hist.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
