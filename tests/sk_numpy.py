"""The model of the static structure factor (include/nbco.h, nbco_structure_factor) that the tests hold the library to.

t_a = (double) x_a * (kstep_a / 6.283185307179586) and r_a = t_a - rint(t_a) are formed as the rule forms them, in fp64; both are what
the library sees, r exactly.  A particle counts iff every t_a is finite.  From there on the model is long double: cos / sin of
2 pi (ix r_x + iy r_y + iz r_z) and the sums over the particles.  No part of the library's polynomial or of its products is repeated
here, so a wrong sign, index, conjugate or a dropped particle shows as an error of order 1, and rounding as one far below the bound."""
import numpy as np

L = np.longdouble
assert np.finfo(L).nmant >= 63, "the model needs a long double with at least 64 bits of mantissa"
TWO_PI_D = 6.283185307179586
TWO_PI = L(8) * np.arctan(L(1))
U = 2.0 ** -53


def count(h):
    h = list(h)
    return (h[0] + 1) * (2 * h[1] + 1) * (2 * h[2] + 1 if len(h) == 3 else 1)


def index(h, ix, iy, iz=0):
    if len(h) == 2:
        return ix * (2 * h[1] + 1) + iy + h[1]
    return (ix * (2 * h[1] + 1) + iy + h[1]) * (2 * h[2] + 1) + iz + h[2]


def bound(n, h):
    """|rho_k(library) - rho_k(model)| <= n u (8 (hx + hy + hz + 1) + n): the base phases (4 u) and one complex product per power step
    and axis join, plus the worst case of any summation order over n terms of modulus <= 1"""
    return n * U * (8.0 * (sum(h) + 1) + n)


def reduced(x, kstep):
    """(r, used): the reduced phases in cycles (fp64, as the rule forms them) of the rows that count, and which rows those are"""
    x = np.asarray(x)
    dim = x.shape[1]
    w = np.array([float(kstep[a]) / TWO_PI_D for a in range(dim)], dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        t = x.astype(np.float64) * w[None, :]
    used = np.isfinite(t).all(axis=1)
    t = t[used]
    return t - np.rint(t), used


def structure_factor(x, h, kstep, chunk=4096, only=None):
    """(re, im, n_used): rho_k of the rows x (n, 2 or 3) as two long double arrays over the K wave vectors of the grid -- or, with
    `only` (an array of flat indices), over those wave vectors alone"""
    h = [int(v) for v in h]
    r, used = reduced(x, kstep)
    dim = r.shape[1]
    ix = np.arange(0, h[0] + 1)
    iy = np.arange(-h[1], h[1] + 1)
    iz = np.arange(-h[2], h[2] + 1) if dim == 3 else np.zeros(1, dtype=np.int64)
    K = count(h)
    re, im = np.zeros(K, dtype=L), np.zeros(K, dtype=L)
    rl = r.astype(L)
    # rows of at most `chunk` particles against a slab of k at a time, to bound the memory
    kx = np.repeat(ix, len(iy) * len(iz)).astype(L)
    ky = np.tile(np.repeat(iy, len(iz)), len(ix)).astype(L)
    kz = np.tile(iz, len(ix) * len(iy)).astype(L)
    if only is not None:
        kx, ky, kz = kx[only], ky[only], kz[only]
        K = len(kx)
        re, im = np.zeros(K, dtype=L), np.zeros(K, dtype=L)
    kslab = max(1, (1 << 21) // max(1, min(chunk, max(1, len(rl)))))
    for k0 in range(0, K, kslab):
        k1 = min(K, k0 + kslab)
        for j0 in range(0, len(rl), chunk):
            b = rl[j0:j0 + chunk]
            cyc = np.outer(kx[k0:k1], b[:, 0]) + np.outer(ky[k0:k1], b[:, 1])
            if dim == 3:
                cyc += np.outer(kz[k0:k1], b[:, 2])
            cyc -= np.rint(cyc)
            ang = TWO_PI * cyc
            re[k0:k1] += np.cos(ang).sum(axis=1)
            im[k0:k1] += np.sin(ang).sum(axis=1)
    return re, im, int(used.sum())


def error(rho, re, im):
    """max over k of |rho_k - model_k|, rho a complex128 array"""
    dr = rho.real.astype(L) - re
    di = rho.imag.astype(L) - im
    return float(np.sqrt(dr * dr + di * di).max())


def cloud(n, seed, sigma=(1.0, 0.6, 1.7), centre=(0.0, 0.0, 0.0), dim=3):
    """a Gaussian ball with unequal axes; float32 rows for dim 3, float64 for dim 2"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)) * np.array(sigma[:dim]) + np.array(centre[:dim])
    return np.ascontiguousarray(x.astype(np.float32 if dim == 3 else np.float64))
