"""numpy fp64 yardsticks of the 2-D energy diagnostics (nbco_2d_energy, nbco_2d_energy_fmm).  Test infrastructure.

    phi_i   = sum_{j != i} 1/2 log(|x_i - x_j|^2 + EPS2)     (j != i by index)
    psi_i   = -param[0] phi_i
    kinetic = 1/2 sum |v|^2,  elastic = 1/2 sum (kx x^2 + ky y^2),  coulomb = 1/2 sum psi_i

`exact` is the all-pairs sum.  `fmm_energy` restates the FMM potential pass in the complex form of fmm2d_numpy: the tree, the
multipoles and the field's locals b_l are those of fmm2d_numpy.fmm, and with W(z) = sum_j log(z - z_j), W' = f, the potential's
local expansion is the field's plus one real constant per cell:

    Re W(u) = c0 + Re sum_{l<p} b_l u^(l+1) / (l+1)
    M2L     c0 += a_0 1/2 log(|D|^2 + EPS2) - Re sum_{k=2..p} a_k w^k / k,   w = conj(D) / (|D|^2 + EPS2)
    L2L     c0_child += c0_parent + Re sum_{l<p} b^parent_l d^(l+1) / (l+1)
    L2P     phi_i = near pairs + c0 + Re sum_l b_l u^(l+1) / (l+1)
"""
import math

import numpy as np

import fmm2d_numpy as F


def kin_ela(x, v, param):
    return 0.5 * float((v * v).sum()), 0.5 * float((x * x * np.array(param[2:4])).sum())


def exact(x, v, param, eps2):
    """all pairs in slabs of 32 targets, numpy's pairwise row sums.  Returns (energies[3], psi[n], abs_rows[n]): abs_rows[i] is
    sum_j |psi_i's pair term|; the sum of |coulomb's pair terms| is abs_rows.sum() / 2."""
    n = len(x)
    xs, ys = x[:, 0].copy(), x[:, 1].copy()
    phi, ab = np.zeros(n), np.zeros(n)
    for s in range(0, n, 32):
        e = min(s + 32, n)
        dx, dy = xs[s:e, None] - xs[None, :], ys[s:e, None] - ys[None, :]
        lg = 0.5 * np.log(dx * dx + dy * dy + eps2)
        lg[np.arange(e - s), np.arange(s, e)] = 0.0
        phi[s:e] = lg.sum(1)
        ab[s:e] = np.abs(lg).sum(1)
    psi = -param[0] * phi
    kin, ela = kin_ela(x, v, param)
    return np.array([kin, ela, 0.5 * float(psi.sum())]), psi, abs(param[0]) * ab


def fmm_energy(state, p, eps2, param, radius=1, dens_inhom=1.0, tree_L=0, near_chunk=F.NEAR_CHUNK):
    """the FMM potential pass.  Returns (energies[3], psi[n] in input order, S) with the scale
    S = |param[0]| / 2 (sum |near pair terms of phi| + sum_i |far_i|) in the units of coulomb."""
    x0, v0 = state[0], state[1]
    n = len(x0)
    L = F.levels(n, p, dens_inhom, tree_L)
    k = F.keys(x0, L, eps2)
    order = np.argsort(k, kind="stable")
    x = x0[order]
    ks = k[order]
    side = 1 << L
    m = side * side
    index = np.searchsorted(ks, np.arange(m + 1), side="left")
    mult = np.diff(index)
    z = x[:, 0] + 1j * x[:, 1]
    # leaves
    cnt = mult.astype(np.float64)
    sz = np.bincount(ks, weights=x[:, 0], minlength=m) + 1j * np.bincount(ks, weights=x[:, 1], minlength=m)
    cen = np.where(mult > 0, sz / np.maximum(cnt, 1), 0)
    w = z - cen[ks]
    mp = np.zeros((m, p + 1), dtype=np.complex128)
    mp[:, 0] = cnt
    pw = w.copy()
    for q in range(2, p + 1):
        pw = pw * w
        mp[:, q] = np.bincount(ks, weights=pw.real, minlength=m) + 1j * np.bincount(ks, weights=pw.imag, minlength=m)
    C = {L: (cen.reshape(side, side), mp.reshape(side, side, p + 1), mult.reshape(side, side))}
    # M2M
    for l in range(L - 1, 1, -1):
        cc, mc, uc = C[l + 1]
        s = 1 << l
        mlt = uc.reshape(s, 2, s, 2).sum(axis=(1, 3))
        wsum = (cc * uc).reshape(s, 2, s, 2).sum(axis=(1, 3))
        ce = np.where(mlt > 0, wsum / np.maximum(mlt, 1), 0)
        M = np.zeros((s, s, p + 1), dtype=np.complex128)
        for di in range(2):
            for dj in range(2):
                a = mc[di::2, dj::2]
                d = np.where(uc[di::2, dj::2] > 0, cc[di::2, dj::2] - ce, 0)
                for q in range(2, p + 1):
                    acc = a[..., 0] * d ** q
                    for r in range(2, q + 1):
                        acc = acc + math.comb(q, r) * a[..., r] * d ** (q - r)
                    M[..., q] += acc
        M[..., 0] = mlt
        C[l] = (ce, M, mlt)
    # M2L: the field's locals and the constant
    loc, c0 = {}, {}
    for l in range(2, L + 1):
        ce, M, mlt = C[l]
        s = 1 << l
        b = np.zeros((s, s, p), dtype=np.complex128)
        c = np.zeros((s, s))
        I, J = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
        im, jm = (I // 2) * 2, (J // 2) * 2
        for ok in range(-2 * radius, 2 * radius + 2):
            for og in range(-2 * radius, 2 * radius + 2):
                K, G = im + ok, jm + og
                ok_ = (K >= 0) & (K < s) & (G >= 0) & (G < s)
                far = (np.abs(K - I) > radius) | (np.abs(G - J) > radius)
                Kc, Gc = np.clip(K, 0, s - 1), np.clip(G, 0, s - 1)
                use = ok_ & far & (mlt > 0) & (mlt[Kc, Gc] > 0)
                if not use.any():
                    continue
                D = (ce - ce[Kc, Gc])[use]
                r2 = D.real ** 2 + D.imag ** 2 + eps2
                wv = np.conj(D) / r2
                a = M[Kc, Gc][use]
                add = np.zeros((len(D), p), dtype=np.complex128)
                for ll in range(p):
                    for kk in [0] + list(range(2, p + 1)):
                        add[:, ll] += (-1) ** ll * math.comb(kk + ll, ll) * a[:, kk] * wv ** (kk + ll + 1)
                b[use] += add
                t = a[:, 0].real * (0.5 * np.log(r2))
                for kk in range(2, p + 1):
                    t = t - (a[:, kk] * wv ** kk).real / kk
                c[use] += t
        loc[l], c0[l] = b, c
    # L2L
    for l in range(3, L + 1):
        ce, _, mlt = C[l]
        cp = np.repeat(np.repeat(C[l - 1][0], 2, 0), 2, 1)
        bp = np.repeat(np.repeat(loc[l - 1], 2, 0), 2, 1)
        c0p = np.repeat(np.repeat(c0[l - 1], 2, 0), 2, 1)
        d = ce - cp
        g = np.zeros_like(d)
        for ll in range(p):
            g = g + bp[..., ll] * d ** (ll + 1) / (ll + 1)
        c0[l] += np.where(mlt > 0, c0p + g.real, 0)
        for mm in range(p):
            acc = np.zeros_like(d)
            for ll in range(mm, p):
                acc = acc + math.comb(ll, mm) * bp[..., ll] * d ** (ll - mm)
            loc[l][..., mm] += np.where(mlt > 0, acc, 0)
    # L2P
    bl = loc[L].reshape(m, p)
    u = z - cen[ks]
    g = np.zeros_like(u)
    for ll in range(p):
        g = g + bl[ks, ll] * u ** (ll + 1) / (ll + 1)
    far = c0[L].reshape(m)[ks] + g.real
    # near field, the self pair excluded by its place in the sorted array
    near, near_abs = np.zeros(n), 0.0
    for c in np.nonzero(mult)[0]:
        i, j = divmod(int(c), side)
        rows = []
        for kr in range(max(i - radius, 0), min(i + radius, side - 1) + 1):
            rows.append(np.arange(index[kr * side + max(j - radius, 0)], index[kr * side + min(j + radius, side - 1) + 1]))
        si = np.concatenate(rows)   # ascending: the rows follow each other in key order
        sx, sy = x[si, 0], x[si, 1]
        b, e = int(index[c]), int(index[c + 1])
        step = e - b if near_chunk is None else max(1, near_chunk // len(si))
        for t in range(b, e, step):
            te = min(t + step, e)
            lg = x[t:te, 0, None] - sx[None, :]
            dy = x[t:te, 1, None] - sy[None, :]
            lg *= lg
            dy *= dy
            lg += dy
            lg += eps2
            np.log(lg, out=lg)
            lg *= 0.5
            lg[np.arange(te - t), np.searchsorted(si, np.arange(t, te))] = 0.0
            near[t:te] = lg.sum(1)
            near_abs += float(np.abs(lg, out=lg).sum())
    phi = near + far
    psi = np.empty(n)
    psi[order] = -param[0] * phi
    kin, ela = kin_ela(x0, v0, param)
    S = 0.5 * abs(param[0]) * (near_abs + float(np.abs(far).sum()))
    return np.array([kin, ela, 0.5 * float(psi.sum())]), psi, S
