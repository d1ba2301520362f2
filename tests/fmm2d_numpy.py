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
    xs, ys = x[:, 0].copy(), x[:, 1].copy()
    # 32 targets a slab keeps the slabs in cache; a contiguous row sum is numpy's pairwise summation, closer to the true sum than a
    # running one
    for s in range(0, n, 32):
        dx, dy = xs[s:s + 32, None] - xs[None, :], ys[s:s + 32, None] - ys[None, :]
        inv = 1.0 / (dx * dx + dy * dy + eps2)
        out[s:s + 32, 0] = (dx * inv).sum(1)
        out[s:s + 32, 1] = (dy * inv).sum(1)
    return out * scale


def direct_rows(x, rows, eps2, scale=1.0):
    """exact sums for the targets `rows` only"""
    out = np.zeros((len(rows), 2))
    for s in range(0, len(rows), 4):
        d = x[rows[s:s + 4]][:, None, :] - x[None, :, :]
        inv = 1.0 / ((d * d).sum(-1) + eps2)
        out[s:s + 4] = (d * inv[..., None]).sum(1)
    return out * scale


NEAR_CHUNK = 1 << 21   # target x source pairs per slab of the near-field loop (three fp64 arrays of 2 x that many values)


def fmm(state, p, eps2, param, radius=1, coll=True, dens_inhom=1.0, tree_L=0, a_in=None, near_chunk=NEAR_CHUNK, m2l_eps2=None):
    """fmm_cart: returns (state in cell order [2, n, 2], accelerations [n, 2]) for state = [positions, velocities].
    near_chunk: the near field of one leaf is summed in slabs of about that many pairs, split over targets only, so every target's
    sum keeps its order (None: one slab per leaf).  m2l_eps2: the softening of the M2L alone, for tests that show what a comparison
    can see (None: eps2, the reference's)."""
    if m2l_eps2 is None:
        m2l_eps2 = eps2
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
                wv = np.conj(D) / (D.real ** 2 + D.imag ** 2 + m2l_eps2)
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
            b, e = int(index[c]), int(index[c + 1])
            step = e - b if near_chunk is None else max(1, near_chunk // len(src))
            for t in range(b, e, step):
                d = x[t:min(t + step, e), None, :] - src[None, :, :]
                inv = 1.0 / ((d * d).sum(-1) + eps2)
                near[t:min(t + step, e)] = (d * inv[..., None]).sum(1)
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


# ---- the integrators by their own properties: order of convergence and time reversal, direct force, n = 64 -----------------------
ORDERS = (1, 1, 2, 4, 4)              # Euler, pre-Euler, leapfrog, Forest-Ruth, PEFRL
REVERSIBLE = (2, 3, 4)
CONV_N, CONV_T, CONV_STEPS, CONV_FINE = 64, 0.04, (16, 32, 64), 4096   # a quarter of a betatron period (1 / 6.2 s)
# EPS2 of the run: sqrt(EPS2) is half a semi-axis, so no pair comes closer than the steps resolve.  At the program's 1e-18 close
# encounters keep every scheme out of its asymptotic regime at these step counts (leapfrog's error ratio is 1.5, not 4).
CONV_EPS2 = float(np.float32(1e-6))


def conv_force(param, eps2):
    """f for integrate(): the exact pair sum times param[0], and the elastic term"""
    k = np.array(param[2:])

    def f(b):
        b[2] = direct(b[0], eps2, param[0]) - k * b[0]
    return f


def conv_start(state, param, eps2):
    """[x, v, a] with a evaluated at x: the Euler variant and the leapfrog kick before their first evaluation"""
    buf = np.concatenate([state, np.zeros_like(state[:1])])
    conv_force(param, eps2)(buf)
    return buf


def conv_dist(a, b):
    """distance of two buffers over positions and velocities, each relative to its own size"""
    return float(max(np.linalg.norm(a[q] - b[q]) / np.linalg.norm(b[q]) for q in (0, 1)))


def conv_ratios(run, buf0, fine):
    """run(scheme, buf, dt, steps) -> buf after `steps` steps.  Returns, per scheme, the errors against `fine` at CONV_STEPS and the
    ratios of neighbouring errors (about 2^order in the asymptotic regime)."""
    out = {}
    for scheme in range(5):
        errs = [conv_dist(run(scheme, buf0.copy(), CONV_T / k, k), fine) for k in CONV_STEPS]
        out[scheme] = (errs, [a / b for a, b in zip(errs, errs[1:])])
    return out


def conv_return(run, negate, buf0, scheme, steps=CONV_STEPS[0]):
    """`steps` steps, velocities negated, `steps` steps: the distance from (x0, -v0)"""
    b = run(scheme, buf0.copy(), CONV_T / steps, steps)
    b = run(scheme, negate(b), CONV_T / steps, steps)
    want = buf0.copy()
    want[1] = -want[1]
    return conv_dist(b, want)


def lattice(n_side):
    """n_side x n_side points on [0, 1]^2, both box edges included (x slowest); velocities are the reversed positions, halved"""
    g = np.arange(n_side, dtype=np.float64) / (n_side - 1)
    X, Y = np.meshgrid(g, g, indexing="ij")
    x = np.stack([X.ravel(), Y.ravel()], 1)
    return np.stack([x, x[::-1] * 0.5])


SHAPES = ("gauss", "line", "clusters", "ring", "lattice", "coincident", "all_coincident")


def shape(kind, n, seed=0):
    """test inputs [2, n, 2] = [positions, velocities] that a uniformly filled ellipse does not give.  Lengths are multiples of the
    KV semi-axes A (velocities of omega A / 2), so that kv_params()'s param keeps its meaning; `lattice` keeps its unit square."""
    A, om, _xi, _ = kv_params()
    A = np.array(A)
    rng = np.random.default_rng([seed, SHAPES.index(kind), n])
    v = rng.normal(size=(n, 2)) * (np.array(om) * A / 2)
    if kind == "gauss":            # crowded centre, empty corners
        x = rng.normal(size=(n, 2)) * (A / 2)
    elif kind == "line":           # flat: one y for every particle
        x = np.stack([rng.uniform(-1.0, 1.0, n) * A[0], np.full(n, 0.3 * A[1])], 1)
    elif kind == "clusters":       # three tight blobs: two a few leaves apart, the third across the box
        c = np.array([[-1.0, -1.0], [1.0, 1.0], [1.0, 0.9]])[np.arange(n) % 3]
        x = (c + 0.01 * rng.normal(size=(n, 2))) * A
    elif kind == "ring":           # thin annulus: the centroid of the upper cells lies in an empty child
        r, t = rng.uniform(0.95, 1.0, n), rng.uniform(0.0, 2 * math.pi, n)
        x = np.stack([r * np.cos(t), r * np.sin(t)], 1) * A
    elif kind == "lattice":
        s = math.isqrt(n)
        assert s * s == n, "lattice: n must be a square"
        return lattice(s)
    elif kind == "coincident":     # three quarters at one point, the rest scattered
        x = rng.normal(size=(n, 2)) * (A / 2)
        x[: 3 * n // 4] = 0.25 * A
        x = x[rng.permutation(n)]
    elif kind == "all_coincident":
        x = np.tile(0.25 * A, (n, 1))
    else:
        raise ValueError(kind)
    return np.stack([x, v])


def _case(shape, n, p, reach, radius=1, L=0, coll=1, dens=1.0, eps2=1e-18, p1=0.0, unit=0):
    return dict(shape=shape, n=n, p=p, radius=radius, L=L, coll=coll, dens=dens, eps2=eps2, p1=p1, unit=unit, reach=reach)


# The inputs of test_gpu_fmm2d.test_fmm_accelerations_match_restatement beyond the KV beam at n = 6000.  `reach` names the property
# of the tree that the case is there for; test_fmm2d_host.test_shape_cases_reach_their_paths proves each on the CPU from levels()
# and keys().  unit = 1 divides the positions by A (a box of a few units), where an EPS2 of 1e-6 .. 1e-4 softens the M2L without
# collapsing the tree: in metres sqrt(EPS2) exceeds the leaf size and the cell-size clamp takes over (reach "clamp").
SHAPE_CASES = (
    [_case("gauss", 30001, 5, "leaf>64"), _case("gauss", 6000, 5, "leaf>256", L=2), _case("gauss", 8000, 8, "leaf>256", radius=2, L=3),
     _case("gauss", 30001, 5, "rows>100", L=2),
     _case("kv", 6000, 4, "leaf>256", L=2), _case("line", 5000, 5, "flat"), _case("line", 5000, 5, "flat", L=6)]
    + [_case("clusters", 9000, 6, "empty>0.9", radius=r, L=L) for r in (1, 2) for L in (0, 7)]
    + [_case("ring", 9000, 6, "hollow")]
    + [_case("lattice", s * s, p, "full", L=L) for s, p in ((64, 5), (65, 3)) for L in (0, 6)]
    + [_case("coincident", 2000, 5, "pile"), _case("all_coincident", 2000, 5, "one_leaf")]
    + [_case("kv", 6000, 5, "stencil", radius=3), _case("kv", 6000, 10, "stencil", radius=2)]
    + [_case("gauss", n, p, "tiny", L=L) for n in (1, 2, 3, 5, 63, 64, 65, 129) for p, L in ((1, 0), (1, 2), (3, 0), (10, 0))]
    + [_case(s, 6000, 5, "clamp", eps2=e) for s in ("kv", "gauss") for e in (1e-6, 1e-4)]
    + [_case(s, 6000, 5, "soft_m2l", eps2=e, unit=1) for s in ("kv", "gauss") for e in (1e-6, 1e-4)]
    + [_case("gauss", 6000, 5, "nocoll", coll=0, p1=0.37)])


def case_state(cfg, kv):
    """the input of one case; kv(n) supplies the KV beam (the library's host initialiser)"""
    st = kv(cfg["n"]) if cfg["shape"] == "kv" else shape(cfg["shape"], cfg["n"])
    if cfg.get("unit"):
        st = st.copy()
        st[0] /= np.array(kv_params()[0])
    return st


def case_id(c):
    return "%(shape)s%(n)d_p%(p)d_r%(radius)d_L%(L)d_coll%(coll)d_eps%(eps2)g_u%(unit)d" % c


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
