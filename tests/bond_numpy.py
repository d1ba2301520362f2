"""fp64 model of the bond-orientational order (nbco_bond_order / nbco_bond_order_tree / nbco_2d_bond_order), independent of the
library's harmonics.  The neighbour rule is that of include/nbco.h verbatim: d = (double) x_j - (double) x_i per axis;
r2 = (dx dx + dy dy) + dz dz (2-D: dx dx + dy dy), every product and sum a numpy fp64 operation of its own, so rounded once; j is a
neighbour of i iff 0 < r2 < rmax * rmax.  Per particle, by the addition theorem, q_l^2 = (1 / nb^2) sum_{j,k} P_l(u_ij . u_ik): a Legendre
double sum over the bonds, no spherical harmonic anywhere.  The global Q_l^2 is the same double sum over ALL bonds of the cloud, taken
through the monomial moments M_abc = sum x^a y^b z^c: sum_{b,b'} (u_b . u_b')^k = sum_{a+b+c=k} k!/(a! b! c!) M_abc^2, accumulated in
long double.  2-D: psi_l = |sum (u_x + i u_y)^l| / nb from numpy's complex powers.  The model returns the SQUARES: the tests compare
squares, whose error bound (1e-11 for nb <= 256) is derived in tests/test_gpu_bond_order.py."""
import math

import numpy as np

TOL2 = 1e-11          # |delta q_l^2|, |delta psi_l^2|, |delta Q_l^2| for nb <= 256
TOL_MEAN = math.sqrt(TOL2)   # of a mean of q_l: for a, b >= 0, |a - b| <= sqrt(|a^2 - b^2|), and a mean errs no more than its worst term
LEG = {4: {4: 35.0 / 8, 2: -30.0 / 8, 0: 3.0 / 8}, 6: {6: 231.0 / 16, 4: -315.0 / 16, 2: 105.0 / 16, 0: -5.0 / 16}}   # P_l(t) = sum c_k t^k


def legendre(l, t):
    c = LEG[l]
    t2 = t * t
    if l == 4:
        return (c[4] * t2 + c[2]) * t2 + c[0]
    return ((c[6] * t2 + c[4]) * t2 + c[2]) * t2 + c[0]


def bonds(pos, rmax, chunk=256):
    """(i, d, r2) of all directed bonds i -> j, sorted by i (and by j within i): i int64[B], d float64[B, D] = x_j - x_i, r2 float64[B]"""
    x = np.asarray(pos).astype(np.float64)
    n = x.shape[0]
    R2 = float(rmax) * float(rmax)
    I, Dv, R = [np.zeros(0, dtype=np.int64)], [np.zeros((0, x.shape[1]))], [np.zeros(0)]
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, n, chunk):
            d = x[None, :, :] - x[lo:lo + chunk, None, :]
            r2 = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]
            if x.shape[1] == 3:
                r2 = r2 + d[:, :, 2] * d[:, :, 2]
            a, b = np.nonzero((0.0 < r2) & (r2 < R2))
            I.append(a + lo); Dv.append(d[a, b]); R.append(r2[a, b])
    return np.concatenate(I), np.concatenate(Dv), np.concatenate(R)


def _global_q2_3d(u, l):
    """(1 / B^2) sum_{b,b'} P_l(u_b . u_b') through the monomial moments, in long double"""
    B = len(u)
    if B == 0:
        return 0.0
    w = u.astype(np.longdouble)
    total = np.longdouble(0)
    for k, ck in LEG[l].items():
        s = np.longdouble(0)
        for a in range(k + 1):
            for b in range(k + 1 - a):
                c = k - a - b
                m = (w[:, 0] ** a * w[:, 1] ** b * w[:, 2] ** c).sum()
                s += np.longdouble(math.factorial(k) // (math.factorial(a) * math.factorial(b) * math.factorial(c))) * m * m
        total += np.longdouble(ck) * s
    return float(total / (np.longdouble(B) * np.longdouble(B)))


def bond_order(pos, rmax):
    """dict of nb int64[n], q2 float64[n, 2] (q4^2, q6^2; 2-D psi4^2, psi6^2; 0 where nb = 0), bonds, isolated, nb_max,
    q_mean[2] (the mean of sqrt(q2) over nb > 0, 0 if none) and Q2[2] (the global Q_l^2, 0 if there is no bond)"""
    x = np.asarray(pos)
    n, dim = x.shape
    i, d, r2 = bonds(x, rmax)
    u = d * (1.0 / np.sqrt(r2))[:, None]
    nb = np.bincount(i, minlength=n).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(nb)])
    q2 = np.zeros((n, 2))
    for p in np.nonzero(nb)[0]:
        v = u[start[p]:start[p + 1]]
        if dim == 3:
            g = v @ v.T
            q2[p] = [legendre(4, g).sum(), legendre(6, g).sum()]
        else:
            z = v[:, 0] + 1j * v[:, 1]
            q2[p] = [abs((z ** 4).sum()) ** 2, abs((z ** 6).sum()) ** 2]
        q2[p] /= float(nb[p]) ** 2
    q2 = np.maximum(q2, 0.0)   # (a double sum that is 0 in exact arithmetic may come out as -1e-17)
    B = len(i)
    if dim == 3:
        Q2 = [_global_q2_3d(u, 4), _global_q2_3d(u, 6)]
    else:
        z = (u[:, 0] + 1j * u[:, 1]).astype(np.clongdouble)
        Q2 = [float(abs((z ** l).sum()) ** 2 / np.longdouble(B) ** 2) if B else 0.0 for l in (4, 6)]
    linked = nb > 0
    q_mean = np.sqrt(q2[linked]).mean(axis=0) if linked.any() else np.zeros(2)
    return dict(nb=nb, q2=q2, bonds=int(nb.sum()), isolated=int((nb == 0).sum()), nb_max=int(nb.max()), q_mean=q_mean, Q2=np.maximum(np.array(Q2), 0.0))


def global_q2_double_sum(pos, rmax, l):
    """the global Q_l^2 as the plain Legendre double sum over all bonds: what the moment form above is checked against (small clouds)"""
    _, d, r2 = bonds(pos, rmax)
    if len(d) == 0:
        return 0.0
    u = d * (1.0 / np.sqrt(r2))[:, None]
    return float(legendre(l, u @ u.T).sum() / float(len(u)) ** 2)


# ---- ideal lattices with integer fp32 coordinates; the particle at the origin is `centre` -----------------------------------------
def _grid(h):
    g = np.arange(-h, h + 1)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def _shuffled(pts, seed):
    pts = pts[np.random.default_rng(seed).permutation(len(pts))]
    centre = int(np.nonzero((pts == 0).all(axis=1))[0][0])
    return pts.astype(np.float32), centre


def sc(h=6, seed=11):
    """simple cubic, spacing 1, (2h + 1)^3 points (h = 6: 2197)"""
    return _shuffled(_grid(h), seed)


def bcc(g=4, seed=12):
    """body-centred cubic: the corners 2k and the centres 2k + 1 for k in [-g, g): 2 (2g)^3 points (g = 4: 1024)"""
    k = np.arange(-g, g)
    c = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    return _shuffled(np.concatenate([2 * c, 2 * c + 1]), seed)


def fcc(h=4, seed=13):
    """face-centred cubic: the integer points of [-h, h]^3 with an even coordinate sum (h = 4: 365)"""
    p = _grid(h)
    return _shuffled(p[p.sum(axis=1) % 2 == 0], seed)


# (lattice, rmax^2, nb, q4, q6) of the central particle; Steinhardt, Nelson and Ronchetti, Phys. Rev. B 28, 784, table I.  The values hold to 1e-7.
IDEAL = [
    ("sc", 1.5, 6, math.sqrt(7.0 / 12.0), math.sqrt(1.0 / 8.0)),
    ("bcc", 3.5, 8, 0.50917508, 0.62853936),
    ("bcc", 4.5, 14, 0.03636965, 0.51068823),
    ("fcc", 3.0, 12, 0.19094065, 0.57452426),
]
LATTICES = {"sc": sc, "bcc": bcc, "fcc": fcc}


def square2d(side=7):
    g = np.arange(side, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2), (side // 2) * side + side // 2


def triangular2d(side=7):
    """rows of spacing sqrt(3) / 2, every other row shifted by 1 / 2 (fp64 carries the sqrt(3) / 2)"""
    r, c = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    pts = np.stack([c + 0.5 * (r % 2), r * (math.sqrt(3.0) / 2.0)], axis=-1).reshape(-1, 2)
    return pts, (side // 2) * side + side // 2
