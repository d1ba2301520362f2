"""fp64 restatement of the 3-D potential pass (nbco_kd_potential, csrc/kd_potential_kernels.hpp) in numpy, with explicit multi-index
loops and none of the generated operator text: what the device kernels and gen_ops.py's lpot_body are compared against.

A tree is a dict of arrays as Engine.kd_array / Oracle.kd_tree return them: "L", "center" [ntot, 3], "mult", "index" [ntot],
"mpole" [ntot, p(p+1)(p+2)/6], "local" [ntot, (p+1)^2], "p2p" and "m2l" [pairs, 2] (unordered pairs of node numbers; a leaf's own
pair is implied).  Positions are in tree order.  Conventions (csrc/gen_ops.py): a symmetric rank-n tensor is stored with z as the
outer index, x descending; multipoles M[K] = (-1)^n / n! sum_j d_j^K; locals L_n = F_n / n! with F_n the n-th derivative tensor
of the far potential at the node centre, of which only the components with z <= 1 are stored (the trace vanishes).
"""
from math import factorial

import numpy as np


def sym_off(n):
    return n * (n + 1) * (n + 2) // 6


def tl_off(n):
    return n * n


def comps(n):
    """(x, y, z) of a rank-n symmetric tensor in storage order"""
    return [(x, n - x - z, z) for z in range(n + 1) for x in range(n - z, -1, -1)]


def expand_traceless(local, p):
    """{(x, y, z): F[..]} for 1 <= x + y + z <= p from traceless tuples local[.., (p + 1)^2]"""
    local = np.asarray(local, dtype=np.float64)
    F = {}
    for n in range(1, p + 1):
        for z in (0, 1):
            for x in range(n - z, -1, -1):
                F[(x, n - x - z, z)] = local[..., tl_off(n) + (z + 1) * n - x] * float(factorial(n))
        for z in range(2, n + 1):
            for x in range(n - z, -1, -1):
                y = n - x - z
                F[(x, y, z)] = -(F[(x + 2, y, z - 2)] + F[(x, y + 2, z - 2)])
    return F


def taylor_inv_r(d, eps2, kmax):
    """{K: b_K[..]} for |K| <= kmax, b_K = (d/dx)^K (|x|^2 + eps2)^(-1/2) / K! at x = d[.., 3]
    (k R^2 b_K + (2k - 1) sum_a d_a b_{K - e_a} + (k - 1) sum_a b_{K - 2 e_a} = 0, k = |K|, R^2 = |d|^2 + eps2)"""
    d = np.asarray(d, dtype=np.float64)
    R2 = (d * d).sum(-1) + eps2
    b = {(0, 0, 0): 1.0 / np.sqrt(R2)}
    for k in range(1, kmax + 1):
        for K in comps(k):
            t1 = np.zeros_like(R2)
            t2 = np.zeros_like(R2)
            for a in range(3):
                if K[a] >= 1:
                    Km = list(K); Km[a] -= 1
                    t1 = t1 + d[..., a] * b[tuple(Km)]
                if K[a] >= 2:
                    Km = list(K); Km[a] -= 2
                    t2 = t2 + b[tuple(Km)]
            b[K] = -((2 * k - 1) * t1 + (k - 1) * t2) / (k * R2)
    return b


def m2p(mpole, d, eps2, p):
    """potential of multipole tuples mpole[.., offM(p)] (orders 0 .. p-1) at the offsets d[.., 3] from their centres"""
    mpole = np.asarray(mpole, dtype=np.float64)
    b = taylor_inv_r(d, eps2, p - 1)
    phi = np.zeros(np.asarray(d).shape[:-1], dtype=np.float64)
    for k in range(p):
        s = np.zeros_like(phi)
        for i, K in enumerate(comps(k)):
            s = s + mpole[..., sym_off(k) + i] * b[K]
        phi = phi + float(factorial(k)) * s
    return phi


def lpot(F, d, p):
    """sum_{1 <= |K| <= p} d^K / K! F[K]: the far potential at centre + d less its value at the centre"""
    d = np.asarray(d, dtype=np.float64)
    phi = np.zeros(np.broadcast(d[..., 0], F[(1, 0, 0)]).shape, dtype=np.float64)
    for n in range(1, p + 1):
        for (x, y, z) in comps(n):
            mono = d[..., 0] ** x * d[..., 1] ** y * d[..., 2] ** z / float(factorial(x) * factorial(y) * factorial(z))
            phi = phi + mono * F[(x, y, z)]
    return phi


def node_c0(tree, p, eps2):
    """far potential at every node centre: the node's own M2L sources evaluated there, plus the parent's expansion at the centre"""
    C = np.asarray(tree["center"], dtype=np.float64)
    M = np.asarray(tree["mpole"], dtype=np.float64)
    ntot = len(C)
    pairs = np.asarray(tree["m2l"], dtype=np.int64).reshape(-1, 2)
    tgt = np.concatenate([pairs[:, 0], pairs[:, 1]])
    src = np.concatenate([pairs[:, 1], pairs[:, 0]])
    c0 = np.zeros(ntot, dtype=np.float64)
    if len(tgt):
        c0 += np.bincount(tgt, weights=m2p(M[src], C[tgt] - C[src], eps2, p), minlength=ntot)
    F = expand_traceless(tree["local"], p)
    for l in range(1, int(tree["L"]) + 1):
        ch = np.arange((1 << l) - 1, (2 << l) - 1)
        par = (ch - 1) >> 1
        c0[ch] = (c0[ch] + c0[par]) + lpot({K: v[par] for K, v in F.items()}, C[ch] - C[par], p)
    return c0


def leaf_neighbours(tree, coll=True):
    """per leaf (0 .. 2^L - 1): the leaves of its P2P range, itself included"""
    L = int(tree["L"])
    first, nleaf = (1 << L) - 1, 1 << L
    nb = [[lf] if coll else [] for lf in range(nleaf)]
    if coll:
        for a, b in np.asarray(tree["p2p"], dtype=np.int64).reshape(-1, 2) - first:
            nb[a].append(int(b))
            nb[b].append(int(a))
    return nb


class Potential:
    """phi(x) as a particle of leaf `lf` sees it: pair sum over the leaf's P2P range + c0[leaf] + lpot(F[leaf], x - c_leaf)"""

    def __init__(self, tree, pos, p, eps2, coll=True):
        self.tree, self.p, self.eps2 = tree, p, float(eps2)
        self.pos = np.asarray(pos, dtype=np.float64)
        self.C = np.asarray(tree["center"], dtype=np.float64)
        self.first = (1 << int(tree["L"])) - 1
        self.c0 = node_c0(tree, p, self.eps2)
        self.F = expand_traceless(tree["local"], p)
        self.nb = leaf_neighbours(tree, coll)
        self.index, self.mult = np.asarray(tree["index"]), np.asarray(tree["mult"])

    def sources(self, lf):
        idx = [np.arange(self.index[self.first + s], self.index[self.first + s] + self.mult[self.first + s]) for s in self.nb[lf]]
        return np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64)

    def near(self, lf, X, self_idx):
        src = self.sources(lf)
        if not len(src):
            return np.zeros(len(X))
        d = X[:, None, :] - self.pos[src][None, :, :]
        w = 1.0 / np.sqrt((d * d).sum(-1) + self.eps2)
        w[np.asarray(self_idx)[:, None] == src[None, :]] = 0.0     # j != i by index
        return w.sum(1)

    def far(self, lf, X):
        leaf = self.first + lf
        return self.c0[leaf] + lpot({K: v[leaf] for K, v in self.F.items()}, X - self.C[leaf], self.p)

    def at(self, lf, X, self_idx):
        X = np.asarray(X, dtype=np.float64)
        return self.near(lf, X, self_idx) + self.far(lf, X)

    def parts(self):
        """(near_i, far_i) of every particle, tree order: phi_i = near_i + far_i"""
        near, far = np.zeros(len(self.pos)), np.zeros(len(self.pos))
        for lf in range(self.first + 1):
            i0, m = self.index[self.first + lf], self.mult[self.first + lf]
            idx = np.arange(i0, i0 + m)
            near[idx], far[idx] = self.near(lf, self.pos[idx], idx), self.far(lf, self.pos[idx])
        return near, far

    def all(self):
        """phi_i of every particle, tree order"""
        near, far = self.parts()
        return near + far


def psi(tree, pos, p, eps2, param0, coll=True):
    """psi_i = param0 phi_i in tree order"""
    return float(param0) * Potential(tree, pos, p, eps2, coll).all()


def psi_parts(tree, pos, p, eps2, param0, coll=True):
    """(param0 near_i, param0 far_i) in tree order: the pair sum over the leaf's P2P range and c0[leaf] + lpot; psi_i is their sum"""
    near, far = Potential(tree, pos, p, eps2, coll).parts()
    return float(param0) * near, float(param0) * far


def m2l_sources(tree):
    """(start, src): the M2L sources of node v are src[start[v]:start[v + 1]], both directions of every unordered pair"""
    ntot = len(tree["center"])
    pairs = np.asarray(tree["m2l"], dtype=np.int64).reshape(-1, 2)
    tgt = np.concatenate([pairs[:, 0], pairs[:, 1]])
    src = np.concatenate([pairs[:, 1], pairs[:, 0]])
    order = np.argsort(tgt, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=ntot))])
    return start, src[order]


def restated_energy_fmm(tree, pos, p, eps2, param0, coll=True):
    """The Coulomb energy as kd_potential_kernel (csrc/kd_energy_kernels.hpp, nbco_energy_fmm) forms it: per particle the pair sum
    over its leaf's P2P range (j != i by index) plus m2p of every M2L source of the leaf and of each of its ancestors, evaluated AT
    THE PARTICLE; param0 / 2 times the sum.  No locals are read, and a particle's leaf is the one whose index / mult range holds
    it -- the kernel's (2^L i) / n is not restated."""
    x = np.asarray(pos, dtype=np.float64)
    C = np.asarray(tree["center"], dtype=np.float64)
    M = np.asarray(tree["mpole"], dtype=np.float64)
    index, mult = np.asarray(tree["index"]), np.asarray(tree["mult"])
    first = (1 << int(tree["L"])) - 1
    nb = leaf_neighbours(tree, coll)
    start, srcs = m2l_sources(tree)
    seen = np.zeros(len(x), dtype=np.int64)
    total = 0.0
    for lf in range(first + 1):
        idx = np.arange(index[first + lf], index[first + lf] + mult[first + lf])
        if not len(idx):
            continue
        seen[idx] += 1
        X = x[idx]
        phi = np.zeros(len(idx))
        near = [np.arange(index[first + s], index[first + s] + mult[first + s]) for s in nb[lf]]
        if near:
            j = np.concatenate(near)
            d = X[:, None, :] - x[j][None, :, :]
            w = 1.0 / np.sqrt((d * d).sum(-1) + float(eps2))
            w[idx[:, None] == j[None, :]] = 0.0
            phi += w.sum(1)
        chain, node = [], first + lf
        while True:
            chain.append(srcs[start[node]:start[node + 1]])
            if node == 0:
                break
            node = (node - 1) >> 1
        s = np.concatenate(chain)
        if len(s):
            phi += m2p(M[s][None, :, :], X[:, None, :] - C[s][None, :, :], float(eps2), p).sum(1)
        total += phi.sum()
    assert (seen == 1).all(), "the leaves' index / mult ranges hold every particle once"
    return 0.5 * float(param0) * total


def pair_potential(pos, eps2):
    """exact phi_i = sum_{j != i by index} (|x_i - x_j|^2 + eps2)^(-1/2), fp64, in row blocks"""
    x = np.asarray(pos, dtype=np.float64)
    n = len(x)
    out = np.zeros(n)
    for s in range(0, n, 512):
        d = x[s:s + 512, None, :] - x[None, :, :]
        w = 1.0 / np.sqrt((d * d).sum(-1) + float(eps2))
        w[np.arange(len(w)), np.arange(s, s + len(w))] = 0.0
        out[s:s + 512] = w.sum(1)
    return out
