#!/usr/bin/env python3
"""Times of the slice diagnostics on one context: nbco_slice_moments with 16, 256 and 4096 slices along z over
+-3 sigma, beside the yardsticks of the same state -- nbco_beam_moments and a 256-bin nbco_hist along z -- and what a user does
without them: the state copied to the host and the slices taken there (tests/slice_numpy.py, timed once: it takes seconds).
Median of 5 each, at N = 65 536 and 2^20, on the Gaussian ball bench.py uses.  Every timed call ends synchronised, so wall time
around it is the time of the call.  Writes profiles/r11a_slice_moments.json.

    python tools/bench_slice_moments.py [--sizes 65536 1048576] [--slices 16 256 4096] [--repeats 5] [--no-host] [--out FILE]

NBCO_LIB=<library> times another build of the same ABI (the values of kSliceChunk tried; give such a run an --out of its own:
profiles/r11b_slice_moments_variants.json collects them); `chunk` in the output is read from the source tree and describes the
default library only."""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, repeats):
    fn()                                   # (buffers sized, kernels loaded)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def once_ms(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 1 << 20])
    ap.add_argument("--slices", type=int, nargs="+", default=[16, 256, 4096])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11a_slice_moments.json"))
    a = ap.parse_args()
    import torch
    import bench
    import slice_numpy
    from coulomb_oscillators_amd import Engine, Q_Z, lib_path
    src = open(os.path.join(ROOT, "coulomb_oscillators_amd", "csrc", "slice_diag_kernels.hpp")).read()
    chunk = int(re.search(r"constexpr int kSliceChunk = (\d+);", src).group(1))
    rows = []
    eng = Engine(sync=1)
    for n in a.sizes:
        d = torch.from_numpy(bench.gaussian_ball(n)).cuda()
        m = eng.beam_moments(d, n)
        sd = m.cov[Q_Z][Q_Z] ** 0.5
        win = (m.mean[Q_Z] - 3 * sd, m.mean[Q_Z] + 3 * sd)
        counts = torch.empty(257, dtype=torch.int64, device="cuda")
        row = {"n": n, "repeats": a.repeats, "chunk": chunk, "library": os.path.basename(lib_path())}
        row["moments_ms"] = median_ms(lambda: eng.beam_moments(d, n), a.repeats)
        row["profile_256_ms"] = median_ms(lambda: eng.hist(d, n, [(Q_Z, 256) + win], counts), a.repeats)
        for s in a.slices:
            axis = (Q_Z, s) + win
            row["slices_%d_ms" % s] = median_ms(lambda: eng.slice_moments(d, n, axis), a.repeats)
            row["slices_%d_over_moments" % s] = row["slices_%d_ms" % s] / row["moments_ms"]
            recs, outside = eng.slice_moments(d, n, axis)
            row["slices_%d_fullest" % s], row["slices_%d_outside" % s] = max(r.n for r in recs), outside
            if not a.no_host:
                row["host_slices_%d_ms" % s] = once_ms(lambda: slice_numpy.slice_moments(d[:2].cpu().numpy(), 3, axis))
        row["host_copy_ms"] = median_ms(lambda: d[:2].cpu(), a.repeats)
        rows.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_slice_moments.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
