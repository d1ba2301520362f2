#!/usr/bin/env python3
"""Times of the tracked trajectories and their time correlations on one context.

nbco_traj_record at N = 2^20 with stride 1 and 16 (identity numbers, and a random permutation as `ids`), beside nbco_minmax over the
same positions as the one-pass yardstick.  nbco_time_corr at rows = 2^12 and 2^16 with frames = lags = 256 and 1024 on random walks
with random velocities (every frame finite).  One warm-up call per shape, then the repeats alternate between the shapes of one group;
median, minimum and maximum of the repeats and their spread (max - min) / median.  The engine runs with sync = 1, so every timed
call ends synchronised and wall time around it is the time of the call.  `terms` is rows * lags * (2 frames - lags + 1) / 2, the
number of (row, origin, lag) triples; the rule spends 13 fp64 vector instructions on each (3 subtractions, 1 multiplication, 9 fused
multiply-adds) besides the 6 conversions of frame t + tau, so `fp64_fraction` is 13 terms / time over the card's fp64 vector issue
rate, 256 CUs x 64 lanes per clock x 2.4 GHz = 39.3e12 per second -- the figure tools/bench_structure_factor.py uses.  With
--host the host route -- copy the buffer, the same sums in fp64 numpy lag by lag -- is timed once at the smallest case.
Writes profiles/r12a_time_corr.json.

    python tools/bench_time_corr.py [--repeats 7] [--no-host] [--out profiles/r12a_time_corr.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_LANES_PER_S = 256 * 64 * 2.4e9
FP64_PER_TERM = 13


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def stats(v):
    med = statistics.median(v)
    return {"ms": med, "min_ms": min(v), "max_ms": max(v), "spread": (max(v) - min(v)) / med}


def host_route(traj, frames, lags):
    """what a user does without the call: copy, then per lag the differences and products of whole arrays in fp64 numpy"""
    import numpy as np
    t = traj.cpu().numpy()[:, :frames].astype(np.float64)
    x, v = t[..., :3], t[..., 3:]
    out = np.zeros((lags, 8))
    for tau in range(lags):
        m = frames - tau
        d = x[:, tau:] - x[:, :m]
        ok = np.isfinite(t[:, tau:]).all(axis=2) & np.isfinite(t[:, :m]).all(axis=2)
        d2 = np.where(ok[..., None], d * d, 0.0)
        out[tau, :3] = d2.sum(axis=(0, 1))
        out[tau, 3] = (d2.sum(axis=2) ** 2).sum()
        out[tau, 4:7] = np.where(ok[..., None], v[:, tau:] * v[:, :m], 0.0).sum(axis=(0, 1))
        out[tau, 7] = ok.sum()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12a_time_corr.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from coulomb_oscillators_amd import Engine, CORR_LAG
    rows_out = []
    eng = Engine(sync=1)

    # ---- recording ----------------------------------------------------------------------------------------------------------------
    n = 1 << 20
    state = torch.cat([torch.from_numpy(bench.gaussian_ball(n)[0].copy()).reshape(-1), torch.randn(6 * n)]).cuda()
    perm = torch.randperm(n, device="cuda").to(torch.int32)
    cap = 4
    bufs = {s: torch.empty(((n + s - 1) // s, cap, 6), dtype=torch.float32, device="cuda") for s in (1, 16)}
    calls = {"minmax": lambda: eng.minmax(state, n)}
    for s in (1, 16):
        calls["record stride %d" % s] = lambda s=s: eng.traj_record(state, n, bufs[s], 1, stride=s)
        calls["record stride %d, permuted ids" % s] = lambda s=s: eng.traj_record(state, n, bufs[s], 2, stride=s, ids=perm)
    for f in calls.values():
        f()
    ts = {k: [] for k in calls}
    for _ in range(a.repeats):
        for k, f in calls.items():
            ts[k].append(timed_ms(f))
    for k in calls:
        row = {"what": k, "n": n, "repeats": a.repeats, **stats(ts[k])}
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    del bufs, state

    # ---- correlation --------------------------------------------------------------------------------------------------------------
    for lg in (12, 16):
        rows = 1 << lg
        cap = 1024
        traj = torch.empty((rows, cap, 6), dtype=torch.float32, device="cuda")
        traj[..., :3] = torch.cumsum(0.05 * torch.randn((rows, cap, 3), device="cuda"), dim=1)
        traj[..., 3:] = torch.randn((rows, cap, 3), device="cuda")
        shapes = (256, 1024)
        out = {f: torch.empty((f, 8), dtype=torch.float64, device="cuda") for f in shapes}
        for f in shapes:
            eng.time_corr(traj, rows, f, f, out=out[f])
        ts = {f: [] for f in shapes}
        for _ in range(a.repeats):
            for f in shapes:
                ts[f].append(timed_ms(lambda: eng.time_corr(traj, rows, f, f, out=out[f])))
        for f in shapes:
            terms = rows * f * (f + 1) // 2
            st = stats(ts[f])
            rec = out[f].cpu().numpy().view(CORR_LAG).reshape(-1)
            row = {"what": "time_corr", "rows": rows, "frames": f, "lags": f, "frames_cap": cap, "repeats": a.repeats, **st, "terms": terms,
                   "gterms_per_s": 1e-6 * terms / st["ms"], "fp64_fraction": FP64_PER_TERM * terms / (1e-3 * st["ms"]) / FP64_LANES_PER_S,
                   "pairs_lag0": int(rec["pairs"][0]), "msd_lag1": float(rec["dx2"][1].sum() / rec["pairs"][1])}
            if lg == 12 and f == 256 and not a.no_host:
                t0 = time.perf_counter()
                ref = host_route(traj, f, f)
                row["host_route_ms"] = 1e3 * (time.perf_counter() - t0)
                got = out[f].cpu().numpy()
                row["host_route_max_rel_diff_dx2"] = float(np.abs(ref[1:, :3] / got[1:, :3] - 1.0).max())
            rows_out.append(row)
            print(json.dumps(row), flush=True)
        del traj
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_time_corr.py", "device": torch.cuda.get_device_name(0), "rows": rows_out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
