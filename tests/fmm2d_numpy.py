"""numpy fp64 restatement of the reference's 2-D program (Simulation/main.cu, DIM 2, SCAL double): the pair law, `fmm_cart`
(fmm_cart.cuh:395-544) and the integrators (integrator.cuh:32-167).  Test infrastructure, written from the reference's definitions.

The expansions are written in complex form: a 2-D traceless tensor of order k has two components, one complex number.  With
z = x + iy and f(z) = sum_j 1 / (z - z_j), the field d / |d|^2 (d = x_i - x_j) is conj(f(z_i)).
  multipole about c:  a_k = sum_j (z_j - c)^k, k = 0 and 2..p (the dipole vanishes about the centroid and is not computed)
  local about c:      f(z) = sum_l b_l (z - c)^l, l = 0..p-1 (the field terms of the reference's local orders 1..p)
  M2L:                b_l += (-1)^l C(k+l, l) a_k w^(k+l+1), w = conj(D) / (|D|^2 + EPS2), D = c_target - c_source,
                      for k = 0..p, l = 0..p-1 (square truncation, total order 1..2p: fmm_cart_base.cuh:757-798)
"""
import math

import numpy as np

TH = 1.3512071919596576340476878089715                     # integrator.cuh:98
XI, LA, CH = 0.1786178958448091, -0.2123418310626054, -0.06626458266981849   # :130-132


def levels(n, p, dens_inhom=1.0, tree_L=0):
    """fmm_cart.cuh:415-417 with std::round (half away from zero); 2 <= L <= 15"""
    if tree_L:
        return tree_L
    v = math.log2(float(np.float32(dens_inhom)) * n / (p * math.sqrt(p))) / 2
    L = int(math.copysign(math.floor(abs(v) + 0.5), v))
    return min(max(L, 2), 15)


def keys(x, L, eps2):
    """integer cell keys ix * side + iy, x slowest (appel.cuh:44-55, fmm_cart.cuh:476-481)"""
    side = 1 << L
    mn, mx = x.min(axis=0), x.max(axis=0)
    delta = max(mx[0] - mn[0], mx[1] - mn[1]) / side
    eps = math.sqrt(eps2)
    if delta < eps:
        delta = eps
    rd = 1.0 / delta
    ix = np.clip(((x[:, 0] - mn[0]) * rd).astype(np.int64), 0, side - 1)
    iy = np.clip(((x[:, 1] - mn[1]) * rd).astype(np.int64), 0, side - 1)
    return ix * side + iy


def direct(x, eps2, scale=1.0):
    """exact all-pairs sum of d / (|d|^2 + EPS2), then * scale"""
    n = len(x)
    out = np.zeros_like(x)
    for s in range(0, n, 1024):
        d = x[s:s + 1024, None, :] - x[None, :, :]
        inv = 1.0 / ((d * d).sum(-1) + eps2)
        out[s:s + 1024] = (d * inv[..., None]).sum(1)
    return out * scale


def direct_rows(x, rows, eps2, scale=1.0):
    """exact sums for the targets `rows` only"""
    out = np.zeros((len(rows), 2))
    for s in range(0, len(rows), 4):
        d = x[rows[s:s + 4]][:, None, :] - x[None, :, :]
        inv = 1.0 / ((d * d).sum(-1) + eps2)
        out[s:s + 4] = (d * inv[..., None]).sum(1)
    return out * scale


def fmm(state, p, eps2, param, radius=1, coll=True, dens_inhom=1.0, tree_L=0, a_in=None):
    """fmm_cart: returns (state in cell order [2, n, 2], accelerations [n, 2]) for state = [positions, velocities]"""
    x0 = state[0]
    n = len(x0)
    L = levels(n, p, dens_inhom, tree_L)
    k = keys(x0, L, eps2)
    order = np.argsort(k, kind="stable")
    st = state[:, order]
    x = st[0]
    ks = k[order]
    side = 1 << L
    m = side * side
    index = np.searchsorted(ks, np.arange(m + 1), side="left")
    mult = np.diff(index)
    z = x[:, 0] + 1j * x[:, 1]
    # leaves: centroid and multipoles (appel.cuh:222-258, fmm_cart.cuh:68-96)
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
    # M2M (fmm_cart.cuh:116-188)
    for l in range(L - 1, 1, -1):
        cc, mc, uc = C[l + 1]
        s = 1 << l
        mu = uc.reshape(s, 2, s, 2)
        mlt = mu.sum(axis=(1, 3))
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
    # M2L (fmm_cart.cuh:214-262)
    loc = {}
    for l in range(2, L + 1):
        ce, M, mlt = C[l]
        s = 1 << l
        b = np.zeros((s, s, p), dtype=np.complex128)
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
                wv = np.conj(D) / (D.real ** 2 + D.imag ** 2 + eps2)
                a = M[Kc, Gc][use]
                add = np.zeros((len(D), p), dtype=np.complex128)
                for ll in range(p):
                    for kk in [0] + list(range(2, p + 1)):
                        add[:, ll] += (-1) ** ll * math.comb(kk + ll, ll) * a[:, kk] * wv ** (kk + ll + 1)
                b[use] += add
        loc[l] = b
    # L2L (fmm_cart.cuh:288-334)
    for l in range(3, L + 1):
        ce, _, mlt = C[l]
        cp = np.repeat(np.repeat(C[l - 1][0], 2, 0), 2, 1)
        bp = np.repeat(np.repeat(loc[l - 1], 2, 0), 2, 1)
        d = ce - cp
        for mm in range(p):
            acc = np.zeros_like(d)
            for ll in range(mm, p):
                acc = acc + math.comb(ll, mm) * bp[..., ll] * d ** (ll - mm)
            loc[l][..., mm] += np.where(mlt > 0, acc, 0)
    # near field (appel.cuh:260-303) and L2P (fmm_cart.cuh:353-376), then rescale
    bl = loc[L].reshape(m, p)
    u = z - cen[ks]
    f = bl[ks, p - 1]
    for q in range(p - 2, -1, -1):
        f = f * u + bl[ks, q]
    far = np.stack([f.real, -f.imag], axis=1)
    if coll:
        near = np.zeros_like(x)
        for c in np.nonzero(mult)[0]:
            i, j = divmod(int(c), side)
            rows = []
            for kr in range(max(i - radius, 0), min(i + radius, side - 1) + 1):
                rows.append(np.arange(index[kr * side + max(j - radius, 0)], index[kr * side + min(j + radius, side - 1) + 1]))
            src = x[np.concatenate(rows)]
            d = x[index[c]:index[c + 1], None, :] - src[None, :, :]
            inv = 1.0 / ((d * d).sum(-1) + eps2)
            near[index[c]:index[c + 1]] = (d * inv[..., None]).sum(1)
    else:
        near = (np.zeros_like(x) if a_in is None else a_in) * param[1]
    return st, (near + far) * param[0]


def mean_relerr(x, ref):
    """reductions.cuh:37-42 rel_diff1, averaged over particles"""
    d2 = ((x - ref) ** 2).sum(1)
    return float(np.mean(np.sqrt(np.maximum(d2 / ((ref * ref).sum(1) + 1e-18), 0))))


def integrate(scheme, buf, f, dt, scale=1.0, steps=1):
    """integrator.cuh:32-167 on buf = [x, v, a] (each [n, 2]); f(buf) evaluates a in place (and may re-order the state)"""
    def K(s):
        buf[1] += buf[2] * s

    def D(s):
        buf[0] += buf[1] * s
    for _ in range(steps):
        if scheme == 0:
            K(dt * scale); D(dt); f(buf)
        elif scheme == 1:
            f(buf); K(dt * scale); D(dt)
        elif scheme == 2:
            ds = dt * scale * 0.5
            K(ds); D(dt); f(buf); K(ds)
        elif scheme == 3:
            ds = dt * scale
            D(dt * TH / 2); f(buf)
            K(ds * TH); D(dt * (1 - TH) / 2); f(buf)
            K(ds * (1 - 2 * TH)); D(dt * (1 - TH) / 2); f(buf)
            K(ds * TH); D(dt * TH / 2)
        else:
            ds = dt * scale
            D(dt * XI); f(buf)
            K(ds * (1 - 2 * LA) / 2); D(dt * CH); f(buf)
            K(ds * LA); D(dt * (1 - 2 * (CH + XI))); f(buf)
            K(ds * LA); D(dt * CH); f(buf)
            K(ds * (1 - 2 * LA) / 2); D(dt * XI)
    return buf


def kv_params():
    """main.cu:271-313: semi-axes A, depressed phase advances omega, perveance xi, and omega0"""
    twopi = 2 * math.pi
    om0 = (6.22 * twopi, 6.21 * twopi)
    emit = (0.03e-3, 0.01e-3)
    omy = 0.8 * om0[1]
    Ay = 2 * math.sqrt(emit[1] / omy)
    A2 = Ay * Ay
    domy = (om0[1] + omy) * (om0[1] - omy)
    om0x2 = om0[0] * om0[0]
    om0x4 = om0x2 * om0x2
    om0x6 = om0x4 * om0x2
    p = -2 * om0x2
    d = -A2 * domy * domy / (4 * emit[0])
    q = d
    D0 = 16 * om0x4
    D1 = 27 * d * d + 128 * om0x6
    Q = np.cbrt((D1 + math.sqrt((27 * d * d + 256 * om0x6) * (27 * d * d))) / 2)
    S = math.sqrt((-2 * p + (Q + D0 / Q)) / 3) / 2
    omx = S - math.sqrt(-4 * S * S - 2 * p - q / S) / 2
    Ax = 2 * math.sqrt(emit[0] / omx)
    xi = domy * Ay * (Ax + Ay) / 2
    return (Ax, Ay), (omx, omy), xi, om0
