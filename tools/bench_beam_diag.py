#!/usr/bin/env python3
"""Times of the beam diagnostics on one context: nbco_beam_moments, a 256-bin profile, a 64 x 64 map (LDS form),
a 1024 x 1024 map (global atomics), the yardstick Engine.pow_sum(x, 2, n) (one 12 B / particle pass with the same reduction
pattern), and what a user does without them: the state copied to the host and the moments taken with numpy.  Median of 5 each, at
N = 65 536 and 2^20, on the Gaussian ball bench.py uses.  Every timed call ends synchronised, so wall time around it is the time of
the call.  `gbps` is the bytes the pass has to read (24 B per particle and pass for the moments, 4 B per particle and axis for a
histogram, 12 B for pow_sum) over that time.  Writes profiles/r08a_beam_diag.json.

    python tools/bench_beam_diag.py [--sizes 65536 1048576] [--repeats 5] [--out profiles/r08a_beam_diag.json]
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


def numpy_moments(state, n):
    """the moments a user takes on the host today: means, central covariance, central fourth-order sums per plane, in fp64"""
    import numpy as np
    q = np.concatenate([state[0], state[1]], axis=1).astype(np.float64)
    d = q - q.mean(0)
    cov = d.T @ d / n
    m4 = [[(d[:, k] ** (4 - j) * d[:, 3 + k] ** j).mean() for j in range(5)] for k in range(3)]
    return cov, m4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 1 << 20])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08a_beam_diag.json"))
    a = ap.parse_args()
    import torch
    import bench
    from coulomb_oscillators_amd import Engine, Q_X, Q_Y, Q_VX
    rows = []
    eng = Engine(sync=1)
    for n in a.sizes:
        d = torch.from_numpy(bench.gaussian_ball(n)).cuda()
        m = eng.beam_moments(d, n)
        win = {c: (m.mean[c] - 4 * m.cov[c][c] ** 0.5, m.mean[c] + 4 * m.cov[c][c] ** 0.5) for c in (Q_X, Q_Y, Q_VX)}
        counts = {k: torch.empty(b + 1, dtype=torch.int64, device="cuda") for k, b in (("profile", 256), ("map64", 64 * 64), ("map1024", 1024 * 1024))}
        calls = {
            "moments": (lambda: eng.beam_moments(d, n), 48 * n),
            "profile_256": (lambda: eng.hist(d, n, [(Q_X, 256) + win[Q_X]], counts["profile"]), 4 * n),
            "map_64x64": (lambda: eng.hist(d, n, [(Q_X, 64) + win[Q_X], (Q_VX, 64) + win[Q_VX]], counts["map64"]), 8 * n),
            "map_1024x1024": (lambda: eng.hist(d, n, [(Q_X, 1024) + win[Q_X], (Q_Y, 1024) + win[Q_Y]], counts["map1024"]), 8 * n),
            "pow_sum": (lambda: eng.pow_sum(d, 2, n), 12 * n),
        }
        row = {"n": n, "repeats": a.repeats}
        for name, (fn, nbytes) in calls.items():
            row[name + "_ms"] = median_ms(fn, a.repeats)
            row[name + "_gbps"] = nbytes / row[name + "_ms"] * 1e-6
        row["host_copy_numpy_ms"] = median_ms(lambda: numpy_moments(d[:2].cpu().numpy(), n), a.repeats)
        row["host_copy_ms"] = median_ms(lambda: d[:2].cpu(), a.repeats)
        row["moments_over_pow_sum"] = row["moments_ms"] / row["pow_sum_ms"]
        row["host_over_moments"] = row["host_copy_numpy_ms"] / row["moments_ms"]
        for k, c in counts.items():
            row[k + "_inside"] = int(c[:-1].sum())
        row["emit_x"], row["halo_x"] = m.emit[0], m.halo[0]
        rows.append(row)
        print(json.dumps(row))
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_beam_diag.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
