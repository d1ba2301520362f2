#!/usr/bin/env python3
"""Times of the collective modes on one context.

Recording: nbco_modes_record beside nbco_structure_factor on the Gaussian ball bench.py uses, positions and velocities, at
N = 2^14, 2^18 and 2^20 and h = (4,4,4) and (8,8,8), kstep = 2 pi / (8 sigma) per axis.  One warm-up call per shape, then the repeats
alternate between the two calls and the grids of one N; median, minimum and maximum of the repeats and their spread
(max - min) / median.  Every timed call ends synchronised (n_used is asked for), so wall time around it is the time of the call.
`terms` is N K; the accumulation loop of the modes spends 12 fp64 vector instructions on each (one complex product: 2 multiplications
and 2 fused multiply-adds; 2 additions; 6 fused multiply-adds), that of the structure factor 6, so `fp64_fraction` is 12 (6) terms / time
over the card's fp64 vector issue rate, 256 CUs x 64 lanes per clock x 2.4 GHz = 39.3e12 per second.  `ratio_to_sk` is the time of
the modes over the time of the structure factor at the same n and grid in the same run.  With --host-log2 the host route -- copy the
state, exp(i k . x) in fp64 numpy, the four sums -- is timed once at that N and the first grid.

Correlation: nbco_mode_corr on a random series at K of h = (4,4,4) and (8,8,8) with frames = lags = 256 and 1024, the engine
synchronous.  `terms` is K lags (2 frames - lags + 1) / 2, the (k, origin, lag) triples; each costs 20 fp64 vector instructions
(P of the later frame: 2 multiplications and 4 fused multiply-adds; rr 2, jj 6, ll 2 fused multiply-adds; 4 additions).
Writes profiles/r13a_modes.json.

    python tools/bench_modes.py [--log2 14 18 20] [--repeats 7] [--host-log2 14] [--out profiles/r13a_modes.json]
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

GRIDS = [(4, 4, 4), (8, 8, 8)]
CORR_SHAPES = [256, 1024]
FP64_LANES_PER_S = 256 * 64 * 2.4e9


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def stats(v):
    med = statistics.median(v)
    return {"ms": med, "min_ms": min(v), "max_ms": max(v), "spread": (max(v) - min(v)) / med}


def host_route(d, n, h, kstep):
    """what a user does without the call: copy, n x K complex exponentials in fp64 numpy, the four sums, in slabs of k"""
    import numpy as np
    s = d.cpu().numpy()
    x, v = s[:3 * n].reshape(n, 3).astype(np.float64), s[3 * n:6 * n].reshape(n, 3).astype(np.float64)
    ix, iy, iz = np.arange(0, h[0] + 1), np.arange(-h[1], h[1] + 1), np.arange(-h[2], h[2] + 1)
    k = np.stack(np.meshgrid(ix * kstep[0], iy * kstep[1], iz * kstep[2], indexing="ij"), axis=-1).reshape(-1, 3)
    out = np.empty((len(k), 4), dtype=np.complex128)
    slab = max(1, (1 << 22) // n)
    for k0 in range(0, len(k), slab):
        e = np.exp(1j * (k[k0:k0 + slab] @ x.T))
        out[k0:k0 + slab, 0] = e.sum(axis=1)
        out[k0:k0 + slab, 1:] = e @ v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[14, 18, 20])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-log2", type=int, default=14)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13a_modes.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from coulomb_oscillators_amd import Engine
    record_rows, corr_rows = [], []
    eng = Engine(sync=1)
    kstep = [2.0 * math.pi / (8.0 * s) for s in bench.SIGMA_X]
    for lg in a.log2:
        n = 1 << lg
        d = torch.from_numpy(bench.gaussian_ball(n).copy()).cuda().reshape(-1)   # [pos | vel | acc]
        K = {h: (h[0] + 1) * (2 * h[1] + 1) * (2 * h[2] + 1) for h in GRIDS}
        series = {h: torch.empty((K[h], 1, 8), dtype=torch.float64, device="cuda") for h in GRIDS}
        rho = {h: torch.empty(K[h], dtype=torch.complex128, device="cuda") for h in GRIDS}
        used = {}
        calls = {("modes", h): (lambda h=h: used.__setitem__(h, eng.modes_record(d, n, h, kstep, series=series[h])[1])) for h in GRIDS}
        calls.update({("sk", h): (lambda h=h: eng.structure_factor(d, n, h, kstep, rho=rho[h])) for h in GRIDS})
        for fn in calls.values():
            fn()                                  # (buffers sized, kernels loaded)
        ts = {key: [] for key in calls}
        for _ in range(a.repeats):
            for key, fn in calls.items():
                ts[key].append(timed_ms(fn))
        for h in GRIDS:
            m, s = stats(ts[("modes", h)]), stats(ts[("sk", h)])
            rec = series[h].cpu().numpy()[:, 0, :]
            row = {"n": n, "h": list(h), "K": K[h], "kstep": kstep, "repeats": a.repeats, "n_used": used[h], **m,
                   "sk_ms": s["ms"], "sk_spread": s["spread"], "ratio_to_sk": m["ms"] / s["ms"], "terms": n * K[h],
                   "fp64_fraction": 12.0 * n * K[h] / (1e-3 * m["ms"]) / FP64_LANES_PER_S,
                   "sk_fp64_fraction": 6.0 * n * K[h] / (1e-3 * s["ms"]) / FP64_LANES_PER_S,
                   "rho_max_diff_to_sk": float(np.abs((rec[:, 0] + 1j * rec[:, 1]) - rho[h].cpu().numpy()).max())}
            if lg == a.host_log2 and h == GRIDS[0]:
                t0 = time.perf_counter()
                ref = host_route(d, n, h, kstep)
                row["host_route_ms"] = 1e3 * (time.perf_counter() - t0)
                row["host_route_max_diff"] = float(np.abs(ref - (rec[:, 0::2] + 1j * rec[:, 1::2])).max())
            record_rows.append(row)
            print(json.dumps(row), flush=True)
    for h in GRIDS:
        Kh = (h[0] + 1) * (2 * h[1] + 1) * (2 * h[2] + 1)
        ser = torch.from_numpy(np.random.default_rng(Kh).standard_normal((Kh, max(CORR_SHAPES), 8))).cuda()
        out = {f: torch.empty((Kh, f, 8), dtype=torch.float64, device="cuda") for f in CORR_SHAPES}
        for f in CORR_SHAPES:
            eng.mode_corr(ser, h, kstep, f, f, out=out[f])
        ts = {f: [] for f in CORR_SHAPES}
        for _ in range(a.repeats):
            for f in CORR_SHAPES:
                ts[f].append(timed_ms(lambda: eng.mode_corr(ser, h, kstep, f, f, out=out[f])))
        for f in CORR_SHAPES:
            terms = Kh * f * (f + 1) // 2
            m = stats(ts[f])
            row = {"h": list(h), "K": Kh, "frames": f, "lags": f, "repeats": a.repeats, **m, "terms": terms,
                   "gterms_per_s": 1e-6 * terms / m["ms"], "fp64_fraction": 20.0 * terms / (1e-3 * m["ms"]) / FP64_LANES_PER_S}
            corr_rows.append(row)
            print(json.dumps(row), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_modes.py", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
                   "record": record_rows, "corr": corr_rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
