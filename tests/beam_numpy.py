"""fp64 numpy reference of the beam diagnostics (include/nbco.h: nbco_beam_moments, nbco_hist and their 2-D forms).

A state is [pos n x D | vel n x D]; q = (x.., v..) are its 2 D phase-space coordinates, in this order.  Sums go through
math.fsum (exactly rounded), so the reference's own error is one rounding per sum plus the roundings of the terms."""
import math

import numpy as np


def phase_space(state, dim):
    """state: anything that reshapes to [2, n, dim] (positions, velocities) -> float64 [n, 2 dim], widened exactly"""
    s = np.asarray(state).reshape(2, -1, dim)
    return np.concatenate([s[0], s[1]], axis=1).astype(np.float64)


def fmean(terms):
    return math.fsum(terms.tolist()) / len(terms)


def moments(state, dim):
    """dict with the fields of nbco_moments (arrays sized as in the C structure, unused entries 0) plus `scale`: for every sum field
    the mean absolute value of the sum's terms, the yardstick of a summation-error bound"""
    q = phase_space(state, dim)
    n, Q = q.shape
    out = dict(n=n, dim=dim, mean=np.zeros(6), min=np.zeros(6), max=np.zeros(6), cov=np.zeros((6, 6)), m4=np.zeros((3, 5)))
    scale = dict(mean=np.zeros(6), cov=np.zeros((6, 6)), m4=np.zeros((3, 5)))
    out["min"][:Q], out["max"][:Q] = q.min(0), q.max(0)
    for a in range(Q):
        # a coordinate that is the same in every particle is its own mean (the header's convention: its deviations are exactly 0)
        out["mean"][a] = q[0, a] if out["min"][a] == out["max"][a] else fmean(q[:, a])
        scale["mean"][a] = fmean(np.abs(q[:, a]))
    d = q - out["mean"][:Q]
    for a in range(Q):
        for b in range(a, Q):
            t = d[:, a] * d[:, b]
            out["cov"][a, b] = out["cov"][b, a] = fmean(t)
            scale["cov"][a, b] = scale["cov"][b, a] = fmean(np.abs(t))
    for k in range(dim):
        x, e = d[:, k], d[:, dim + k]
        for j, t in enumerate((x ** 4, x ** 3 * e, x ** 2 * e ** 2, x * e ** 3, e ** 4)):
            out["m4"][k, j] = fmean(t)
            scale["m4"][k, j] = fmean(np.abs(t))
    out.update(derived(out["cov"], out["m4"], dim))
    out["scale"] = scale
    return out


def derived(cov, m4, dim):
    """emit, halo_q, halo from the central moments, with the zero conventions: halo_q = 0 where <d^2> = 0, emit = halo = 0 where
    I2 = <d^2><e^2> - <d e>^2 <= 0"""
    emit, halo_q, halo = np.zeros(3), np.zeros(3), np.zeros(3)
    for k in range(dim):
        x2, e2, xe = float(cov[k][k]), float(cov[dim + k][dim + k]), float(cov[k][dim + k])
        f = [float(v) for v in m4[k]]
        i2 = x2 * e2 - xe * xe
        i4 = f[0] * f[4] + 3.0 * f[2] * f[2] - 4.0 * f[3] * f[1]
        if x2 > 0.0:
            halo_q[k] = f[0] / (x2 * x2) - 2.0
        if i2 > 0.0:
            emit[k] = math.sqrt(i2)
            halo[k] = math.sqrt(3.0 * max(i4, 0.0)) / (2.0 * i2) - 2.0
    return dict(emit=emit, halo_q=halo_q, halo=halo)


def coord_index(coord, dim):
    """column of phase_space for an NBCO_Q_* number (X, Y, Z, VX, VY, VZ = 0..5); None if the state has no such coordinate"""
    if coord in (0, 1, 2) and coord < dim:
        return coord
    if coord in (3, 4, 5) and coord - 3 < dim:
        return dim + coord - 3
    return None


def bin_of(q, bins, lo, hi):
    """the bin rule verbatim: scale = bins / (hi - lo) once; inside iff q >= lo and q < hi (a NaN is outside);
    b = (int) ((q - lo) * scale), clamped to bins - 1.  Returns (inside, b), b valid where inside."""
    q = np.asarray(q, dtype=np.float64)
    scale = float(bins) / (float(hi) - float(lo))
    inside = (q >= lo) & (q < hi)
    t = (np.where(inside, q, lo) - lo) * scale      # subtract, then multiply
    b = np.minimum(t.astype(np.int64), bins - 1)    # (astype truncates towards zero, as the C cast does; t >= 0 here)
    return inside, b


def hist(state, dim, axes):
    """int64 [B + 1]: counts over one or two (coord, bins, lo, hi) axes, axis 0 the slow index, the particles outside last"""
    q = phase_space(state, dim)
    inside = np.ones(len(q), dtype=bool)
    flat = np.zeros(len(q), dtype=np.int64)
    B = 1
    for coord, bins, lo, hi in axes:
        ins, b = bin_of(q[:, coord_index(coord, dim)], bins, lo, hi)
        inside &= ins
        flat = flat * bins + b
        B *= bins
    out = np.zeros(B + 1, dtype=np.int64)
    out[:B] = np.bincount(flat[inside], minlength=B)
    out[B] = len(q) - int(inside.sum())
    return out
