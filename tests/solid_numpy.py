"""fp64 model of the crystalline-particle detection (nbco_bond_vectors / nbco_bond_solid and their tree forms), on the bonds of
tests/bond_numpy.py: the neighbour rule is bond_numpy.bonds', and `pairs` adds the far end j of every bond to what that function returns.
The bond vector records are formed from sums of engine.bond_harmonics over the bonds (the harmonics are checked on their own in
tests/test_bond_order_host.py).  The coherence is the rule of include/nbco.h verbatim: 13 elementwise numpy products, then 12 numpy adds
from the left, each an fp64 operation of its own, so rounded once -- xi, n_solid, solid_bonds and xi_max are exact integers of the
records.  The averaged order is returned as SQUARES, like bond_numpy's q2: T is added with numpy's own order of summation, which differs
from the kernels' only by rounding."""
import math

import numpy as np

import bond_numpy as BN

VEC = 24            # doubles of a record: q^_4m in [0, 9), q^_6m in [9, 22), a_4, a_6
Q4, Q6 = 4.0 * math.pi / 9.0, 4.0 * math.pi / 13.0


def pairs(pos, rmax, chunk=256):
    """(i, j) of all directed bonds i -> j by the rule of bond_numpy.bonds, in its order (by i, and by j within i); checked against it"""
    x = np.asarray(pos).astype(np.float64)
    n = x.shape[0]
    R2 = float(rmax) * float(rmax)
    I, J = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, n, chunk):
            d = x[None, :, :] - x[lo:lo + chunk, None, :]
            r2 = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]
            r2 = r2 + d[:, :, 2] * d[:, :, 2]
            a, b = np.nonzero((0.0 < r2) & (r2 < R2))
            I.append(a + lo); J.append(b)
    i, j = np.concatenate(I), np.concatenate(J)
    bi, bd, _ = BN.bonds(pos, rmax, chunk)
    assert np.array_equal(i, bi) and np.array_equal(x[j] - x[i], bd)
    return i, j


def sums(pos, rmax):
    """(nb int64[n], S float64[n, 22]): the sums of the harmonics of engine.bond_harmonics over the bonds of every particle"""
    from coulomb_oscillators_amd import bond_harmonics
    n = len(pos)
    i, d, r2 = BN.bonds(pos, rmax)
    u = d * (1.0 / np.sqrt(r2))[:, None]
    Y = np.array([np.concatenate(bond_harmonics(v)) for v in u]).reshape(len(u), 22)
    S = np.zeros((n, 22))
    np.add.at(S, i, Y)
    return np.bincount(i, minlength=n).astype(np.int64), S


def records(pos, rmax):
    """(nb, vec float64[n, VEC]): the bond vector records from those sums; zeros where nb = 0 or a norm is 0"""
    nb, S = sums(pos, rmax)
    vec = np.zeros((len(nb), VEC))
    for lo, hi, a in ((0, 9, 22), (9, 22, 23)):
        norm = np.sqrt((S[:, lo:hi] ** 2).sum(axis=1))
        ok = (nb > 0) & (norm > 0)
        vec[ok, lo:hi] = S[ok, lo:hi] / norm[ok, None]
        vec[ok, a] = norm[ok] / nb[ok]
    return nb, vec


def coherence(e, f):
    """d6 of record pairs (arrays [..., VEC]): elementwise products, added from the left"""
    t = np.asarray(e)[..., 9:22] * np.asarray(f)[..., 9:22]
    d = t[..., 0]
    for m in range(1, 13):
        d = d + t[..., m]
    return d


def solid(pos, rmax, dmin, xi_min, vec=None):
    """dict of nb, xi int64[n], d6 float64[B] (per directed bond, in the order of `pairs`), qbar2 float64[n, 2] (q-bar_4^2, q-bar_6^2;
    0 where nb = 0), and the summary: bonds, isolated, solid_bonds, n_solid, xi_max, qbar_mean[2] (the mean of sqrt(qbar2) over nb > 0).
    vec: the records to use (the device's, copied back), or None for the model's own."""
    n = len(pos)
    if vec is None:
        _, vec = records(pos, rmax)
    vec = np.asarray(vec, dtype=np.float64).reshape(n, VEC)
    i, j = pairs(pos, rmax)
    nb = np.bincount(i, minlength=n).astype(np.int64)
    d6 = coherence(vec[i], vec[j])
    xi = np.bincount(i[d6 > dmin], minlength=n).astype(np.int64)
    w = np.concatenate([vec[:, 0:9] * vec[:, 22:23], vec[:, 9:22] * vec[:, 23:24]], axis=1)   # a_l q^_lm
    T = w.copy()
    np.add.at(T, i, w[j])
    qbar2 = np.stack([Q4 * (T[:, 0:9] ** 2).sum(axis=1), Q6 * (T[:, 9:22] ** 2).sum(axis=1)], axis=1) / (nb[:, None] + 1.0) ** 2
    qbar2[nb == 0] = 0.0
    linked = nb > 0
    return dict(nb=nb, xi=xi, d6=d6, qbar2=qbar2, bonds=int(nb.sum()), isolated=int((nb == 0).sum()), solid_bonds=int(xi.sum()),
                n_solid=int((xi >= xi_min).sum()), xi_max=int(xi.max()), qbar_mean=np.sqrt(qbar2[linked]).mean(axis=0) if linked.any() else np.zeros(2))


def gas(n=1025, seed=5):
    """a uniform random gas in the unit cube and the radius that takes 12 neighbours on average in the bulk"""
    pos = np.random.default_rng(seed).random((n, 3)).astype(np.float32)
    return pos, (12.0 / (4.0 / 3.0 * math.pi * n)) ** (1.0 / 3.0)


def bcc_in_gas(seed=21):
    """the bcc block of bond_numpy (1024 points in [-8, 7]^3) surrounded by 1024 gas points: uniform in [-14, 13]^3 outside the block
    and its margin of 1.5, fp32; returns (pos, is_lattice)"""
    lat, _ = BN.bcc()
    rng = np.random.default_rng(seed)
    out = np.zeros((0, 3))
    while len(out) < 1024:
        p = rng.uniform(-14.0, 13.0, size=(4096, 3))
        out = np.concatenate([out, p[((p < -9.5) | (p > 8.5)).any(axis=1)]])
    pos = np.concatenate([lat, out[:1024].astype(np.float32)])
    perm = rng.permutation(len(pos))
    return np.ascontiguousarray(pos[perm]), perm < 1024
