"""fp64 reference of the pair statistics (nbco_pair_hist / nbco_pair_hist_tree / nbco_2d_pair_hist), the pair rule of include/nbco.h
verbatim: d_a = (double) x_i[a] - (double) x_j[a]; r2 = (dx dx + dy dy) + dz dz (2-D: dx dx + dy dy), every product and sum a numpy
fp64 operation of its own, so rounded once; inside iff r2 < rmax * rmax; bin = the largest b with (b width)^2 <= r2, width =
rmax / bins.  Chunked over rows: n = 4097 costs a few tens of MB."""
import numpy as np


def edges2(bins, rmax):
    """lower2(b) for b = 0 .. bins (the last one is only an edge for the eye: inside is decided by rmax * rmax)"""
    width = float(rmax) / bins
    e = np.arange(bins + 1) * width
    return e * e


def _r2_rows(x, lo, hi):
    """r2 of the rows lo..hi against all particles; x is (n, D) float64"""
    d = x[lo:hi, None, :] - x[None, :, :]
    s = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]
    if x.shape[1] == 3:
        s = s + d[:, :, 2] * d[:, :, 2]
    return s


def inside_pairs(pos, rmax, chunk=256):
    """(r2 of the unordered pairs i < j inside the window, nn2): the part of the statistics that does not depend on the bins.  nn2
    is float64 of n, +inf where no partner is inside.  pos is (n, 3) or (n, 2), any float type: it is widened first."""
    x = np.asarray(pos).astype(np.float64)
    n = x.shape[0]
    R2 = float(rmax) * float(rmax)
    nn2 = np.full(n, np.inf)
    cols = np.arange(n)
    found = [np.zeros(0)]
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            rows = np.arange(lo, hi)[:, None]
            r2 = _r2_rows(x, lo, hi)
            inside = r2 < R2
            m = inside & (cols[None, :] != rows)
            if m.any():
                nn2[lo:hi] = np.where(m, r2, np.inf).min(axis=1)
            found.append(r2[m & (cols[None, :] > rows)])
    return np.concatenate(found), nn2


def counts_of(r2_inside, n, bins, rmax):
    """int64 counts of bins + 1 from inside_pairs' first result: the pairs per bin, then the pairs outside"""
    e2 = edges2(bins, rmax)
    counts = np.zeros(bins + 1, dtype=np.int64)
    b = np.searchsorted(e2[:bins], r2_inside, side="right") - 1
    counts[:bins] = np.bincount(b, minlength=bins)
    counts[bins] = n * (n - 1) // 2 - len(r2_inside)
    return counts


def pair_hist(pos, bins, rmax, chunk=256):
    """(counts, nn2) of nbco_pair_hist: the unordered pairs i < j per bin, then the pairs outside; the smallest r2 per particle"""
    r2_inside, nn2 = inside_pairs(pos, rmax, chunk)
    return counts_of(r2_inside, len(pos), bins, rmax), nn2


LATTICE_RMAX, LATTICE_BINS = 4.0, 8


def lattice(side=5):
    """the integer lattice {0 .. side - 1}^3 as float32 (n = side^3), shuffled with a fixed seed, and its counts for rmax = 4,
    bins = 8 from exact integer arithmetic: r2 is an integer, the bin edges are k / 2, so the bin is the integer square root of
    4 r2 and a pair is inside iff r2 < 16.  Distances 1, 2, 3 sit exactly on the edges of the bins 2, 4, 6 and belong to them;
    distance 4 is exactly rmax and is outside."""
    import math
    g = np.arange(side)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = pts[np.random.default_rng(7).permutation(len(pts))]
    counts = np.zeros(LATTICE_BINS + 1, dtype=np.int64)
    for i in range(len(pts)):
        d = pts[i + 1:] - pts[i]
        for r2 in (d * d).sum(axis=1).tolist():
            counts[math.isqrt(4 * r2) if r2 < 16 else LATTICE_BINS] += 1
    return pts.astype(np.float32), counts


def pair_hist_loops(pos, bins, rmax):
    """the same by a plain double loop over Python floats (fp64, one operation per rounding): what the vectorised form is checked
    against"""
    x = [[float(np.float64(v)) for v in row] for row in np.asarray(pos)]
    n = len(x)
    width = float(rmax) / bins
    lower2 = [(b * width) * (b * width) for b in range(bins)]
    R2 = float(rmax) * float(rmax)
    counts = [0] * (bins + 1)
    nn2 = [float("inf")] * n
    for i in range(n):
        for j in range(i + 1, n):
            dx, dy = x[i][0] - x[j][0], x[i][1] - x[j][1]
            r2 = dx * dx + dy * dy
            if len(x[i]) == 3:
                dz = x[i][2] - x[j][2]
                r2 = r2 + dz * dz
            if not r2 < R2:
                counts[bins] += 1
                continue
            b = 0
            while b + 1 < bins and lower2[b + 1] <= r2:
                b += 1
            counts[b] += 1
            nn2[i] = min(nn2[i], r2)
            nn2[j] = min(nn2[j], r2)
    return np.array(counts, dtype=np.int64), np.array(nn2)
