"""fp64 restatement of the 3-D probe calls (nbco_probe, nbco_kd_probe; csrc/kd_probe_kernels.hpp) in numpy: the exact sums, and the
tree walk with the acceptance test redone in float32 in the order of kd_probe_admissible, so that every decision of the device
walk is reproduced and the two differ by fp64 rounding alone.

A tree is a dict of arrays as Engine.kd_array / Oracle.kd_tree return them: "L", "center", "lbound", "rbound" [ntot, 3], "mult",
"index" [ntot], "mpole" [ntot, p(p+1)(p+2)/6]; positions are in tree order.  All sums come back WITHOUT the factor param[0].
"""
from functools import lru_cache
from math import factorial

import numpy as np

from energy3d_numpy import comps, sym_off, taylor_inv_r   # (taylor_inv_r: the yardstick of taylor_table below)
from nbutil import _powf

f32 = np.float32


def widen(x):
    """what the device computes on: the float32 values, as doubles"""
    return np.asarray(x, dtype=f32).astype(np.float64)


def exact(pos, probes, eps2, with_abs=False):
    """a[m, 3] = sum_j d (|d|^2 + eps2)^(-3/2), psi[m] = sum_j (|d|^2 + eps2)^(-1/2), d = t_i - x_j, every source at every probe;
    with_abs: also sum_j |d| (|d|^2 + eps2)^(-3/2), the scale of the field sum's rounding"""
    x, t, e = widen(pos).reshape(-1, 3), widen(probes).reshape(-1, 3), float(f32(eps2))
    a, psi, mag = np.zeros((len(t), 3)), np.zeros(len(t)), np.zeros(len(t))
    for s in range(0, len(t), 256):
        d = t[s:s + 256, None, :] - x[None, :, :]
        inv = 1.0 / np.sqrt((d * d).sum(-1) + e)
        psi[s:s + 256] = inv.sum(1)
        a[s:s + 256] = (d * (inv ** 3)[..., None]).sum(1)
        mag[s:s + 256] = (np.linalg.norm(d, axis=-1) * inv ** 3).sum(1)
    return (a, psi, mag) if with_abs else (a, psi)


def adm_table(n, L, p):
    """(lo, Mlo, Mhi) per level, as kd_adm_table fills them: libm's powf on float32 quotients"""
    lo, Mlo, Mhi = [], [], []
    e = f32(1) / f32(3 * p + 6)
    for l in range(L + 1):
        a, b = n >> l, (n + (1 << l) - 1) >> l
        lo.append(a)
        Mlo.append(_powf(f32(a) / f32(n), e) if a > 0 else f32(0))
        Mhi.append(_powf(f32(b) / f32(n), e) if b > 0 else f32(0))
    return lo, Mlo, Mhi


def node_sizes(tree):
    """squared box diagonals in float32, as node_csz computes them"""
    d = np.asarray(tree["rbound"], dtype=f32) - np.asarray(tree["lbound"], dtype=f32)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def admissible(c, sz, M, t32, radius):
    """kd_probe_admissible for one node (centre c, size sz, table entry M, all float32) against the probes t32[.., 3]"""
    dx, dy, dz = t32[:, 0] - c[0], t32[:, 1] - c[1], t32[:, 2] - c[2]
    dist2 = (dx * dx + dy * dy) + dz * dz
    parM = f32(radius) * M
    return (parM * parM) * np.maximum(sz, f32(0)) < dist2


@lru_cache(maxsize=None)
def _tables(k):
    """index tables of order k: for every component K of comps(k) and axis a, where K - e_a sits in comps(k - 1), K - 2 e_a in
    comps(k - 2) and K + e_a in comps(k + 1) (index 0 with weight 0 where the component does not exist), and K_a + 1"""
    pos = {j: {K: i for i, K in enumerate(comps(j))} for j in (k - 2, k - 1, k + 1) if j >= 0}
    cs = comps(k)
    dn1, w1, dn2, w2 = (np.zeros((3, len(cs)), dtype=np.int64) for _ in range(4))
    up, wu = np.zeros((3, len(cs)), dtype=np.int64), np.zeros((3, len(cs)))
    for i, K in enumerate(cs):
        for a in range(3):
            Kp = list(K); Kp[a] += 1
            up[a, i], wu[a, i] = pos[k + 1][tuple(Kp)], K[a] + 1
            if K[a] >= 1:
                Km = list(K); Km[a] -= 1
                dn1[a, i], w1[a, i] = pos[k - 1][tuple(Km)], 1
            if K[a] >= 2:
                Km = list(K); Km[a] -= 2
                dn2[a, i], w2[a, i] = pos[k - 2][tuple(Km)], 1
    return dn1, w1.astype(np.float64), dn2, w2.astype(np.float64), up, wu


def taylor_table(d, eps2, kmax):
    """taylor_inv_r of energy3d_numpy with a whole order per numpy operation: a list B[k][component of comps(k), probe], k <= kmax, of
    b_K = (d/dx)^K (|x|^2 + eps2)^(-1/2) / K! at x = d[m, 3] (test_probe3d_host.py holds the two against each other)"""
    d = np.asarray(d, dtype=np.float64)
    R2 = (d * d).sum(-1) + eps2
    B = [(1.0 / np.sqrt(R2))[None, :]]
    for k in range(1, kmax + 1):
        dn1, w1, dn2, w2, _, _ = _tables(k)
        t1 = sum(d[None, :, a] * (w1[a][:, None] * B[k - 1][dn1[a]]) for a in range(3))
        t2 = sum(w2[a][:, None] * B[k - 2][dn2[a]] for a in range(3)) if k >= 2 else 0.0
        B.append(-((2 * k - 1) * t1 + (k - 1) * t2) / (k * R2[None, :]))
    return B


def m2p_field_potential(M, d, eps2, p):
    """(a[m, 3], psi[m]) of one multipole tuple M[offM(p)] at the offsets d[m, 3] from its centre:
    psi = sum_K M[K] |K|! b_K(d),  a_c = -sum_K M[K] |K|! (K_c + 1) b_{K + e_c}(d)"""
    M = np.asarray(M, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    B = taylor_table(d, eps2, p)
    psi, a = np.zeros(len(d)), np.zeros((len(d), 3))
    for k in range(p):
        Mk = M[sym_off(k):sym_off(k + 1)]
        _, _, _, _, up, wu = _tables(k)
        fk = float(factorial(k))
        psi += fk * (Mk[:, None] * B[k]).sum(0)
        for c in range(3):
            a[:, c] -= fk * ((Mk * wu[c])[:, None] * B[k + 1][up[c]]).sum(0)
    return a, psi


def walk(tree, pos_tree, probes, p, radius, eps2, n):
    """the walk of kd_probe_walk_kernel: depth first from the root, left child first; an accepted inner node contributes its expansion
    at the probe, a leaf always its particles pair by pair (it is not tested), any other node is opened.  Returns (a[m, 3], psi[m],
    accepted[m] = list of node numbers, direct[m] = list of leaf node numbers), each list in walk order."""
    L = int(tree["L"])
    ntot = (2 << L) - 1
    C32 = np.asarray(tree["center"], dtype=f32)
    C = C32.astype(np.float64)
    sz = node_sizes(tree)
    mult, index = np.asarray(tree["mult"], dtype=np.int64), np.asarray(tree["index"], dtype=np.int64)
    mp = np.asarray(tree["mpole"], dtype=np.float64)
    lo, Mlo, Mhi = adm_table(int(n), L, p)
    x = widen(pos_tree).reshape(-1, 3)
    t32 = np.asarray(probes, dtype=f32).reshape(-1, 3)
    t = t32.astype(np.float64)
    e = float(f32(eps2))
    m = len(t)
    a, psi = np.zeros((m, 3)), np.zeros(m)
    accepted, direct = [[] for _ in range(m)], [[] for _ in range(m)]
    stack = [(0, np.arange(m))]
    while stack:
        k, idx = stack.pop()
        lev = (k + 1).bit_length() - 1
        M = Mlo[lev] if mult[k] == lo[lev] else Mhi[lev]
        leaf = 2 * k + 1 >= ntot
        adm = admissible(C32[k], sz[k], M, t32[idx], radius) & (not leaf)       # a leaf is never expanded
        ia, io = idx[adm], idx[~adm]
        if len(ia):
            da, dp = m2p_field_potential(mp[k], t[ia] - C[k], e, p)
            a[ia] += da
            psi[ia] += dp
            for i in ia:
                accepted[i].append(k)
        if not len(io):
            continue
        if leaf:
            src = x[index[k]:index[k] + mult[k]]
            d = t[io, None, :] - src[None, :, :]
            inv = 1.0 / np.sqrt((d * d).sum(-1) + e)
            psi[io] += inv.sum(1)
            a[io] += (d * (inv ** 3)[..., None]).sum(1)
            for i in io:
                direct[i].append(k)
        else:
            stack.append((2 * k + 2, io))
            stack.append((2 * k + 1, io))
    return a, psi, accepted, direct


def probe_sets(pos, seed=0):
    """the four probe sets of the accuracy figures: every 7th particle, 500 points in the particles' box, 500 in 1.5 x the box,
    200 in 10 x the box (float32)"""
    pos = np.asarray(pos, dtype=f32).reshape(-1, 3)
    lo, hi = pos.min(0).astype(np.float64), pos.max(0).astype(np.float64)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rng = np.random.default_rng(seed)
    box = lambda cnt, f: (mid + f * half * rng.uniform(-1, 1, (cnt, 3))).astype(f32)
    return {"particles": pos[::7].copy(), "box": box(500, 1.0), "box1.5": box(500, 1.5), "box10": box(200, 10.0)}


def mean_rel(a, ref):
    """mean_i |a_i - ref_i| / |ref_i| over vectors (rows) or scalars"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if a.ndim == 1:
        return float(np.mean(np.abs(a - ref) / np.abs(ref)))
    return float(np.mean(np.linalg.norm(a - ref, axis=1) / np.linalg.norm(ref, axis=1)))


# Mean relative distance of the walk from the exact sums, (field, potential), per probe set of probe_sets(pos, 3), on the fp64
# oracle's tree of the reference ball in tree order at radius 1; "fmm_kd": the same measure for the oracle's evaluator field at every
# 7th particle.  Measured by tests/test_probe3d_host.py, which holds its measurement to these; tests/test_gpu_probe3d.py holds
# the device calls to the row (20000, 6).  At the particles the self term 1 / sqrt(eps2) is taken out of both potentials first.
FIGURES = {
    (4096, 2): {"particles": (4.2407e-02, 6.1543e-03), "box": (1.3994e-02, 3.0252e-03), "box1.5": (2.1257e-02, 5.4862e-03), "box10": (8.7003e-03, 2.3786e-03), "fmm_kd": 1.2538e-01},
    (4096, 4): {"particles": (1.5216e-03, 1.0776e-04), "box": (7.2957e-04, 1.0496e-04), "box1.5": (2.3280e-03, 2.8489e-04), "box10": (2.5832e-04, 3.5369e-05), "fmm_kd": 1.2843e-02},
    (4096, 6): {"particles": (1.0793e-04, 8.0192e-06), "box": (9.5326e-05, 1.4716e-05), "box1.5": (5.8481e-04, 4.1915e-05), "box10": (2.3594e-05, 1.8859e-06), "fmm_kd": 2.0364e-03},
    (4096, 8): {"particles": (6.3187e-06, 6.7768e-07), "box": (1.9569e-05, 2.7034e-06), "box1.5": (9.9792e-05, 6.7613e-06), "box10": (4.0466e-06, 3.2250e-07), "fmm_kd": 1.6492e-04},
    (4096, 10): {"particles": (1.2767e-06, 1.5125e-07), "box": (5.8711e-06, 6.5710e-07), "box1.5": (3.2385e-05, 1.7903e-06), "box10": (1.0416e-06, 6.4756e-08), "fmm_kd": 5.3282e-05},
    (20000, 2): {"particles": (5.9067e-02, 3.1076e+00), "box": (1.3810e-02, 2.6746e-03), "box1.5": (1.6449e-02, 4.2486e-03), "box10": (6.7606e-03, 1.8535e-03), "fmm_kd": 1.7921e-01},
    (20000, 4): {"particles": (4.3119e-03, 2.6960e-04), "box": (1.1283e-03, 9.8493e-05), "box1.5": (1.3047e-03, 1.5971e-04), "box10": (1.4833e-04, 2.0013e-05), "fmm_kd": 5.2285e-02},
    (20000, 6): {"particles": (3.7771e-04, 1.6067e-05), "box": (1.1150e-04, 8.6933e-06), "box1.5": (2.0587e-04, 1.5679e-05), "box10": (8.7272e-06, 6.8516e-07), "fmm_kd": 1.0875e-02},
    (20000, 8): {"particles": (3.3816e-05, 1.2060e-06), "box": (1.2846e-05, 1.0753e-06), "box1.5": (5.8937e-05, 3.0372e-06), "box10": (1.3469e-06, 8.8322e-08), "fmm_kd": 3.2038e-03},
    (20000, 10): {"particles": (5.3795e-06, 2.0442e-07), "box": (2.8030e-06, 2.3889e-07), "box1.5": (2.3626e-05, 9.6292e-07), "box10": (4.5926e-07, 1.8566e-08), "fmm_kd": 1.5689e-03},
}
