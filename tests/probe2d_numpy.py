"""numpy fp64 yardsticks of the 2-D probe calls (nbco_2d_probe, nbco_2d_probe_fmm).  Test infrastructure, written from the formulas.

Every source x_j counts at every probe t_i (no self exclusion: a probe is not a particle):

    a_i   =  param[0] sum_j d / (|d|^2 + EPS2),   d = t_i - x_j
    psi_i = -param[0] sum_j 1/2 log(|d|^2 + EPS2)

`exact` is the all-pairs sum.  `fmm` restates the FMM call in the complex form of fmm2d_numpy: the quadtree of the SOURCES (level
count from n, keys, centroids, multipoles a_k about the centroids), the probes keyed with the sources' box (points outside are
clamped into the border cells), the near field of the probe's leaf (its 2r+1 neighbour rows), and for every level l = L .. 2 the
M2L stencil of the probe's ancestor cell -- the parent's (4r+2)^2 block minus the cell's own (2r+1)^2 neighbourhood -- with each
source's multipole evaluated at the probe itself:

    D = t_i - c_source,  w = conj(D) / (|D|^2 + EPS2)
    f += a_0 w + sum_{k=2..p} a_k w^(k+1),            field = conj(f)
    W += a_0 1/2 log(|D|^2 + EPS2) - Re sum_{k=2..p} a_k w^k / k

Each level's multipoles are computed directly from the particles about the level's centroids (M2M is exact, so this differs from
a chain of shifts by rounding only), and only occupied cells are held, so a forced deep tree stays affordable.
"""
import math

import numpy as np

from fmm2d_numpy import levels, keys


def exact(x, t, eps2, p0=1.0, slab=1 << 21):
    """all pairs in slabs of probes, numpy's pairwise row sums.  Returns (a[m, 2], psi[m], abs_rows[m]): abs_rows[i] is
    sum_j |psi_i's pair term|."""
    m = len(t)
    xs, ys = x[:, 0].copy(), x[:, 1].copy()
    a, phi, ab = np.zeros((m, 2)), np.zeros(m), np.zeros(m)
    step = max(1, slab // len(x))
    for s in range(0, m, step):
        e = min(s + step, m)
        dx, dy = t[s:e, 0, None] - xs[None, :], t[s:e, 1, None] - ys[None, :]
        r2 = dx * dx + dy * dy + eps2
        a[s:e, 0] = (dx / r2).sum(1)
        a[s:e, 1] = (dy / r2).sum(1)
        lg = 0.5 * np.log(r2)
        phi[s:e] = lg.sum(1)
        ab[s:e] = np.abs(lg).sum(1)
    return a * p0, -p0 * phi, abs(p0) * ab


def _cell_coords(pts, mn, rd, side):
    """f2d_keys_kernel on any points with the SOURCES' scalars: truncate, clip to [0, side - 1]"""
    ix = np.clip(((pts[:, 0] - mn[0]) * rd).astype(np.int64), 0, side - 1)
    iy = np.clip(((pts[:, 1] - mn[1]) * rd).astype(np.int64), 0, side - 1)
    return ix, iy


def fmm(x, t, p, eps2, p0=1.0, radius=1, dens_inhom=1.0, tree_L=0, slab=1 << 21):
    """the FMM probe call: returns (a[m, 2], psi[m]) in the probes' order"""
    n, m = len(x), len(t)
    L = levels(n, p, dens_inhom, tree_L)
    side = 1 << L
    mn, mx = x.min(axis=0), x.max(axis=0)
    delta = max(mx[0] - mn[0], mx[1] - mn[1]) / side
    if delta < math.sqrt(eps2):
        delta = math.sqrt(eps2)
    rd = 1.0 / delta
    sx, sy = _cell_coords(x, mn, rd, side)
    assert np.array_equal(sx * side + sy, keys(x, L, eps2))
    order = np.argsort(sx * side + sy, kind="stable")
    xs, sx, sy = x[order], sx[order], sy[order]
    ks = sx * side + sy
    z = xs[:, 0] + 1j * xs[:, 1]
    px, py = _cell_coords(t, mn, rd, side)
    zt = t[:, 0] + 1j * t[:, 1]

    # near field, leaf by leaf over the leaves that hold probes
    ax, ay, phi = np.zeros(m), np.zeros(m), np.zeros(m)
    pk = px * side + py
    porder = np.argsort(pk, kind="stable")
    uk, first = np.unique(pk[porder], return_index=True)
    last = np.append(first[1:], m)
    for c, b, e in zip(uk, first, last):
        i, j = divmod(int(c), side)
        lo = np.arange(max(i - radius, 0), min(i + radius, side - 1) + 1) * side
        rs = np.searchsorted(ks, lo + max(j - radius, 0), side="left")
        re = np.searchsorted(ks, lo + min(j + radius, side - 1) + 1, side="left")
        si = np.concatenate([np.arange(u, v) for u, v in zip(rs, re)])
        if len(si) == 0:
            continue
        rows = porder[b:e]
        step = max(1, slab // len(si))
        for s in range(0, len(rows), step):
            r = rows[s:s + step]
            dx, dy = t[r, 0, None] - xs[None, si, 0], t[r, 1, None] - xs[None, si, 1]
            r2 = dx * dx + dy * dy + eps2
            ax[r] = (dx / r2).sum(1)
            ay[r] = (dy / r2).sum(1)
            phi[r] = (0.5 * np.log(r2)).sum(1)

    # far field: per level the occupied cells' centroids and multipoles, then the stencil, one offset at a time over all probes
    f = np.zeros(m, dtype=np.complex128)
    W = np.zeros(m)
    for l in range(L, 1, -1):
        sh, sl = L - l, 1 << l
        ck = (sx >> sh) * sl + (sy >> sh)            # ascending: the leaf order refines every level's order
        cells, inv, cnt = np.unique(ck, return_inverse=True, return_counts=True)
        cen = (np.bincount(inv, weights=xs[:, 0]) + 1j * np.bincount(inv, weights=xs[:, 1])) / cnt
        u = z - cen[inv]
        mp = np.zeros((len(cells), p + 1), dtype=np.complex128)
        mp[:, 0] = cnt
        pw = u.copy()
        for q in range(2, p + 1):
            pw = pw * u
            mp[:, q] = np.bincount(inv, weights=pw.real) + 1j * np.bincount(inv, weights=pw.imag)
        ci, cj = px >> sh, py >> sh
        im, jm = (ci // 2) * 2, (cj // 2) * 2
        for ok in range(-2 * radius, 2 * radius + 2):
            for og in range(-2 * radius, 2 * radius + 2):
                K, G = im + ok, jm + og
                use = (K >= 0) & (K < sl) & (G >= 0) & (G < sl) & ((np.abs(K - ci) > radius) | (np.abs(G - cj) > radius))
                want = K * sl + G
                at = np.minimum(np.searchsorted(cells, want), len(cells) - 1)
                use &= cells[at] == want
                if not use.any():
                    continue
                src = at[use]
                D = zt[use] - cen[src]
                r2 = D.real ** 2 + D.imag ** 2 + eps2
                w = np.conj(D) / r2
                a = mp[src]
                fa = a[:, 0] * w
                Wa = a[:, 0].real * (0.5 * np.log(r2))
                for q in range(2, p + 1):
                    fa = fa + a[:, q] * w ** (q + 1)
                    Wa = Wa - (a[:, q] * w ** q).real / q
                f[use] += fa
                W[use] += Wa
    out = np.stack([ax + f.real, ay - f.imag], 1) * p0
    return out, -p0 * (phi + W)
