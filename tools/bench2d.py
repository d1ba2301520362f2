"""2-D program: ms per leapfrog step of the fp64 quadtree FMM (p = 5, KV beam, elastic term), one JSON line.

    python tools/bench2d.py [--steps K] [--warmup W] [--repeats R] [--sizes 30001,1048576,4194304]

Per size: W warm-up steps, then R repeats of K timed steps (HIP events around the K calls); ms_per_step is the median repeat.
near_pairs is the near-field pair count of the final state (sum over leaves of targets x sources in the (2r+1)^2 neighbour
cells, the self pair included), from the cell keys of main.cu's formula.

The energy diagnostics at the same sizes and repeats: energy_fmm_ms is the median time of one nbco_2d_energy_fmm call (it
synchronises; wall clock around the call) and fmm_eval_ms the median of one nbco_2d_fmm evaluation of the same state (HIP events),
energy_over_eval their ratio; energy_exact_ms is one nbco_2d_energy call, at sizes up to --exact-max only (it is O(N^2))."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kv_params():
    twopi = 2 * math.pi
    om0 = (6.22 * twopi, 6.21 * twopi)
    emit = (0.03e-3, 0.01e-3)
    omy = 0.8 * om0[1]
    Ay = 2 * math.sqrt(emit[1] / omy)
    domy = (om0[1] + omy) * (om0[1] - omy)
    o2 = om0[0] * om0[0]
    p, d = -2 * o2, -Ay * Ay * domy * domy / (4 * emit[0])
    Q = np.cbrt((27 * d * d + 128 * o2 ** 3 + math.sqrt((27 * d * d + 256 * o2 ** 3) * (27 * d * d))) / 2)
    S = math.sqrt((-2 * p + (Q + 16 * o2 * o2 / Q)) / 3) / 2
    omx = S - math.sqrt(-4 * S * S - 2 * p - d / S) / 2
    Ax = 2 * math.sqrt(emit[0] / omx)
    return (Ax, Ay), (omx, omy), domy * Ay * (Ax + Ay) / 2, om0


def near_pairs(x, L, eps2, r=1):
    side = 1 << L
    mn, mx = x.min(0), x.max(0)
    delta = max(max(mx - mn) / side, math.sqrt(eps2))
    ij = np.clip(((x - mn) * (1.0 / delta)).astype(np.int64), 0, side - 1)
    cnt = np.zeros((side + 2 * r, side + 2 * r))
    np.add.at(cnt, (ij[:, 0] + r, ij[:, 1] + r), 1)
    box = sum(np.roll(np.roll(cnt, a, 0), b, 1) for a in range(-r, r + 1) for b in range(-r, r + 1))
    return int((cnt * box).sum()), int((cnt > 0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="30001,1048576,4194304")
    ap.add_argument("--exact-max", type=int, default=30001)
    args = ap.parse_args()
    import torch
    from coulomb_oscillators_amd import Engine, EVAL2D_FMM, INTEG_LEAPFROG, init2d
    A, om, xi, om0 = kv_params()
    eps2 = float(np.float32(1e-18))
    out = {"metric": "ms per leapfrog step, 2-D fp64 quadtree FMM p = 5, KV beam, 1 GPU", "cases": []}
    for n in [int(s) for s in args.sizes.split(",")]:
        p = 5
        L = min(max(int(math.floor(math.log2(n / (p * math.sqrt(p))) / 2 + 0.5)), 2), 15)
        eng = Engine(fmm_order=p, tree_radius=1.0, eps2=1e-18, coll=1, dens_inhom=1.0, tree_L=0)
        st = init2d(n, "kv", A, om)
        buf = torch.from_numpy(np.concatenate([st.reshape(-1), np.zeros(2 * n)])).cuda()
        prm = torch.from_numpy(np.array([xi / n, 0.0, om0[0] ** 2, om0[1] ** 2])).cuda()
        eng.compute_force_2d(EVAL2D_FMM, buf, n, prm)
        for _ in range(args.warmup):
            eng.integrate_2d(INTEG_LEAPFROG, EVAL2D_FMM, buf, n, prm, 5e-4)
        reps = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                eng.integrate_2d(INTEG_LEAPFROG, EVAL2D_FMM, buf, n, prm, 5e-4)
            e1.record()
            e1.synchronize()
            reps.append(e0.elapsed_time(e1) / args.steps)
        # the energy pass and one plain evaluation, on the state the timed steps left
        a = buf[4 * n:]
        eng.energy_fmm_2d(buf, n, prm)
        en_ms = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            energies = eng.energy_fmm_2d(buf, n, prm)
            en_ms.append((time.perf_counter() - t0) * 1e3)
        ev_ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.fmm_2d(buf, a, n, prm)
            e1.record()
            e1.synchronize()
            ev_ms.append(e0.elapsed_time(e1))
        exact_ms = None
        if n <= args.exact_max:
            eng.energy_2d(buf, n, prm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            exact = eng.energy_2d(buf, n, prm)
            exact_ms = (time.perf_counter() - t0) * 1e3
        x = buf[:2 * n].view(n, 2).cpu().numpy()
        pairs, occupied = near_pairs(x, L, eps2)
        ms = float(np.median(reps))
        out["cases"].append({"n": n, "L": L, "ms_per_step": ms, "repeats_ms": reps, "near_pairs": pairs, "occupied_leaves": occupied,
                             "pairs_per_occupied_leaf_target": pairs / n, "finite": bool(torch.isfinite(buf).all().item()),
                             "energy_fmm_ms": float(np.median(en_ms)), "fmm_eval_ms": float(np.median(ev_ms)),
                             "energy_over_eval": float(np.median(en_ms) / np.median(ev_ms)), "energy_exact_ms": exact_ms,
                             "energies": [float(v) for v in energies]})
        eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
